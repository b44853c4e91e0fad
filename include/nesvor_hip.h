/*
 * nesvor_hip.h — C ABI of libnesvor_hip.so, the MI355X (gfx950) native backend
 * for the NeSVoR INR-training hot path.
 *
 * Plain C: raw device pointers, sizes and an opaque hipStream_t (void*).  No
 * torch types.  Every entry point enqueues work on `stream` and returns the
 * hipError_t of the launch (0 == hipSuccess); nothing synchronises.
 * All tensors are dense, contiguous, fp32 unless stated otherwise.
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * reference tree, daviddmc/NeSVoR v0.1.0).
 */
#ifndef NESVOR_HIP_H
#define NESVOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NESVOR_MAX_LEVELS 32
#define NESVOR_MAX_MLP_LAYERS 4

/* ABI version; bumped on any signature change (38: nesvor_hashgrid_forward_levels, nesvor_hashgrid_backward_adamw_levels and the
 * timing spans 10 and 11 of nesvor_step_timing_read removed; 37: the device loss scaler). */
int nesvor_hip_abi_version(void);

/* ------------------------------------------------------------------------
 * Rigid-transform conversion.  Replaces the pybind module
 * `nesvor.transform_convert_cuda`
 * (nesvor/transform/transform_convert_cuda.cpp:64-69; kernels
 * transform_convert_cuda_kernel.cu:14-440).
 *   ax  : (n,6)   [rotation vector | translation]
 *   mat : (n,3,4) [R | t]
 * ---------------------------------------------------------------------- */
int nesvor_axisangle2mat_forward(const float* ax, float* mat, int n, void* stream);
int nesvor_axisangle2mat_backward(const float* grad_mat, const float* ax, float* grad_ax, int n, void* stream);
int nesvor_mat2axisangle_forward(const float* mat, float* ax, int n, void* stream);
int nesvor_mat2axisangle_backward(const float* mat, const float* grad_ax, float* grad_mat, int n, void* stream);
/* double-precision variants (the reference dispatches float and double) */
int nesvor_axisangle2mat_forward_f64(const double* ax, double* mat, int n, void* stream);
int nesvor_axisangle2mat_backward_f64(const double* grad_mat, const double* ax, double* grad_ax, int n, void* stream);
int nesvor_mat2axisangle_forward_f64(const double* mat, double* ax, int n, void* stream);
int nesvor_mat2axisangle_backward_f64(const double* mat, const double* grad_ax, double* grad_mat, int n, void* stream);

/* Pose regulariser, forward + gradient in one launch.  Replaces NeSVoR.trans_loss
 * (nesvor/nesvor/models.py:357-363: axisangle2mat x2, RigidTransform.inv/.compose
 * transform.py:44-63, mat2axisangle, and their backwards):
 *   err_k = axisangle(inv(T_init,k) o T_k);  loss = mean(err_R^2) + 1e-3 mean(err_T^2)
 * loss_per_slice (n): each slice's share of the loss (sum == loss);
 * grad_ax (n,6): d loss / d ax. */
int nesvor_trans_loss(const float* ax, const float* ax_init, float* loss_per_slice, float* grad_ax, int n, void* stream);

/* ------------------------------------------------------------------------
 * Slice acquisition forward operator A.  Replaces
 * `nesvor.slice_acq_cuda.forward`
 * (nesvor/slice_acquisition/slice_acq_cuda.cpp:156-161; kernel
 * slice_acq_cuda_kernel.cu:17-171, host :954-991).
 *   transforms (n,3,4) translation in voxel units; vol (D,H,W);
 *   vol_mask (D,H,W) uint8/bool or NULL; slices_mask (n,h,w) uint8/bool or
 *   NULL; psf (d_p,h_p,w_p); slices (n,h,w) out — must be zero-filled by the
 *   caller; slices_weight (n,h,w) out (zero-filled) or NULL.
 * ---------------------------------------------------------------------- */
int nesvor_slice_acq_forward(const float* transforms, const float* vol, const uint8_t* vol_mask,
                             const uint8_t* slices_mask, const float* psf, float* slices, float* slices_weight,
                             int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                             float res_slice, int interp_psf, void* stream);

/* Coverage of the slice-acquisition group against the reference's kernels:
 *   * interp_psf != 0 (nearest-voxel sampling with a re-interpolated PSF) exists in all four reference kernels
 *     (slice_acq_cuda_kernel.cu:72-109 forward, :229-279 and :316-366 backward, :526-572 adjoint, :754-800 adjoint
 *     backward) and is built for all four: the forward through its `interp_psf` argument, the other three through the
 *     `*_interp` entry points further down (per-pixel scatter as the reference formulates it).  No caller in the reference
 *     tree ever switches the mode on (slice_acq.py:40-160, svort/srr.py:37-128 and svort/models.py read it from
 *     params["interp_psf"], which every configuration sets to False).
 *   * double precision is built (the *_f64 entry points below; the reference dispatches float and double).
 *   * PSF size: any (the forward kernel keeps PSFs of up to 1024 taps as an LDS list of their non-zero taps and walks
 *     larger ones in global memory; the others read the dense PSF array).
 *   * volume size: the kernels index voxels with int; every entry point of the group returns hipErrorInvalidValue for
 *     D H W > INT_MAX before anything is launched or written.
 *   * empty stack (n h w = 0): nothing is launched; the backwards zero-fill grad_vol / grad_transforms.
 *
 * Adjoint operator A^T (+ optional equalisation) and backward of A, linear-interpolation mode.
 * Replace `nesvor.slice_acq_cuda.adjoint_forward` / `.backward`
 * (slice_acq_cuda.cpp:156-161; kernels slice_acq_cuda_kernel.cu:472-693 and :173-470).
 * Evaluated as a gather over voxels (no atomics, see csrc/slice_acq.hip).
 *   adjoint_forward: slices (n,h,w) -> vol (D,H,W) overwritten; vol_weight (D,H,W) out or NULL;
 *                    equalize != 0 divides vol by the accumulated weight where it is > 0.
 *   backward       : grad_slices (n,h,w) -> grad_vol (D,H,W) overwritten (or NULL) and
 *                    grad_transforms (n,3,4) overwritten (or NULL).
 *   scratch        : 2*n*h*w floats (adjoint) / n*h*w floats (backward) of device memory. */
int nesvor_slice_acq_adjoint_forward(const float* transforms, const float* psf, const float* slices,
                                     const uint8_t* slices_mask, const uint8_t* vol_mask, float* vol, float* vol_weight,
                                     float* scratch, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                     float res_slice, int equalize, void* stream);
/* Backward of A^T: replaces `nesvor.slice_acq_cuda.adjoint_backward` (slice_acq_cuda.cpp:156-161; kernels
 * slice_acq_cuda_kernel.cu:672-950, host :1079-1131), linear mode.  grad_vol (D,H,W) is divided IN PLACE by
 * max(vol_weight, 1e-3) where vol_weight > 0 when equalize != 0, exactly like the reference; vol is the
 * equalised adjoint output (read only when equalize).  grad_slices (n,h,w) must be zero-filled by the caller
 * (pixels with no PSF weight are left untouched), grad_transforms (n,3,4) is overwritten; either may be NULL. */
int nesvor_slice_acq_adjoint_backward(const float* transforms, float* grad_vol, const float* vol_weight,
                                      const uint8_t* vol_mask, const float* psf, const float* slices,
                                      const uint8_t* slices_mask, const float* vol, float* grad_slices,
                                      float* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h,
                                      int w, float res_slice, int equalize, void* stream);
int nesvor_slice_acq_backward(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf,
                              const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                              float* grad_transforms, float* scratch, int D, int H, int W, int d_p, int h_p, int w_p,
                              int n, int h, int w, float res_slice, void* stream);
/* interp_psf = true for the three operators above (slice_acq_cuda_kernel.cu:229-370, :526-606, :754-836): same argument
 * meaning, no scratch.  The kernels ACCUMULATE (atomics): vol / vol_weight, grad_vol / grad_transforms, grad_slices /
 * grad_transforms must be zero-filled by the caller (as the reference's host functions allocate them); any may be NULL where
 * the operator allows it.  adjoint_forward: equalize != 0 needs vol_weight. */
int nesvor_slice_acq_adjoint_forward_interp(const float* transforms, const float* psf, const float* slices,
                                            const uint8_t* slices_mask, const uint8_t* vol_mask, float* vol, float* vol_weight,
                                            int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                            float res_slice, int equalize, void* stream);
int nesvor_slice_acq_backward_interp(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf,
                                     const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                                     float* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                     float res_slice, void* stream);
int nesvor_slice_acq_adjoint_backward_interp(const float* transforms, float* grad_vol, const float* vol_weight,
                                             const uint8_t* vol_mask, const float* psf, const float* slices,
                                             const uint8_t* slices_mask, const float* vol, float* grad_slices,
                                             float* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p, int n,
                                             int h, int w, float res_slice, int equalize, void* stream);
int nesvor_slice_acq_adjoint_forward_interp_f64(const double* transforms, const double* psf, const double* slices,
                                                const uint8_t* slices_mask, const uint8_t* vol_mask, double* vol,
                                                double* vol_weight, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h,
                                                int w, double res_slice, int equalize, void* stream);
int nesvor_slice_acq_backward_interp_f64(const double* transforms, const double* vol, const uint8_t* vol_mask,
                                         const double* psf, const double* grad_slices, const uint8_t* slices_mask,
                                         double* grad_vol, double* grad_transforms, int D, int H, int W, int d_p, int h_p,
                                         int w_p, int n, int h, int w, double res_slice, void* stream);
int nesvor_slice_acq_adjoint_backward_interp_f64(const double* transforms, double* grad_vol, const double* vol_weight,
                                                 const uint8_t* vol_mask, const double* psf, const double* slices,
                                                 const uint8_t* slices_mask, const double* vol, double* grad_slices,
                                                 double* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p,
                                                 int n, int h, int w, double res_slice, int equalize, void* stream);
/* double-precision variants of the four entry points (the reference dispatches float and double,
 * slice_acq_cuda_kernel.cu:970, :1010, :1046, :1114): same contracts, every float* a double*, res_slice a double. */
int nesvor_slice_acq_forward_f64(const double* transforms, const double* vol, const uint8_t* vol_mask,
                                 const uint8_t* slices_mask, const double* psf, double* slices, double* slices_weight,
                                 int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                 double res_slice, int interp_psf, void* stream);
int nesvor_slice_acq_adjoint_forward_f64(const double* transforms, const double* psf, const double* slices,
                                         const uint8_t* slices_mask, const uint8_t* vol_mask, double* vol, double* vol_weight,
                                         double* scratch, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h, int w,
                                         double res_slice, int equalize, void* stream);
int nesvor_slice_acq_backward_f64(const double* transforms, const double* vol, const uint8_t* vol_mask, const double* psf,
                                  const double* grad_slices, const uint8_t* slices_mask, double* grad_vol,
                                  double* grad_transforms, double* scratch, int D, int H, int W, int d_p, int h_p, int w_p,
                                  int n, int h, int w, double res_slice, void* stream);
int nesvor_slice_acq_adjoint_backward_f64(const double* transforms, double* grad_vol, const double* vol_weight,
                                          const uint8_t* vol_mask, const double* psf, const double* slices,
                                          const uint8_t* slices_mask, const double* vol, double* grad_slices,
                                          double* grad_transforms, int D, int H, int W, int d_p, int h_p, int w_p, int n, int h,
                                          int w, double res_slice, int equalize, void* stream);

/* ------------------------------------------------------------------------
 * Multi-resolution hash-grid encoding.  Replaces `tinycudann.Encoding`
 * (external module; call site nesvor/nesvor/models.py:22-25, config
 * models.py:102-111).  See oracle/hashgrid.py for the algorithm statement.
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t n_levels;
  int32_t n_features;                 /* features per level: 1, 2, 4 or 8 */
  float scale[NESVOR_MAX_LEVELS];     /* fp32 grid scale per level */
  uint32_t res[NESVOR_MAX_LEVELS];    /* vertices per axis */
  uint32_t size[NESVOR_MAX_LEVELS];   /* entries in the level */
  uint32_t offset[NESVOR_MAX_LEVELS]; /* entry offset into the flat table */
  uint32_t hashed[NESVOR_MAX_LEVELS]; /* 1: spatial hash, 0: dense index */
} nesvor_grid_t;

/* layout of the encoded matrix pe / dpe */
#define NESVOR_LAYOUT_ROW_MAJOR 0     /* (N, L*F): what tcnn returns to PyTorch */
#define NESVOR_LAYOUT_FEATURE_MAJOR 1 /* (L*F, N): coalesced producer/consumer layout */
#define NESVOR_LAYOUT_CLUSTERED 4     /* forward only, OR-ed into `layout`: every 256 consecutive points are spatially
                                         clustered (the S PSF samples of a slice pixel are contiguous) - selects the
                                         one-workgroup-per-cloud forward kernel; results do not depend on the hint */
#define NESVOR_LAYOUT_UNCLUSTERED 8   /* backward (owner-computes variants) only, OR-ed into `layout`: consecutive points are NOT
                                         spatially clustered (uniform points, a shuffled batch).  The backward first orders the
                                         points by the cells of a coarse lattice (counting sort, three small launches, scratch
                                         inside `workspace`) and hands every workgroup of the aggregation pass 256 points of
                                         neighbouring cells; the gradients do not depend on the hint beyond the owner pass's
                                         summation order.  Without it the backward assumes what the training step produces:
                                         the S PSF samples of a pixel are contiguous.  tcnn's scatter, which this replaces, is
                                         distribution-agnostic (reference call site nesvor/nesvor/models.py:25). */
#define NESVOR_LAYOUT_DY_SCRATCH 16   /* with NESVOR_LAYOUT_UNCLUSTERED | NESVOR_LAYOUT_FEATURE_MAJOR: the workspace was sized by
                                         nesvor_hashgrid_backward_workspace_bytes_ex(.., the same layout) and has room for dpe
                                         re-ordered into rows (4 L F bytes per point): the aggregation pass then reads whole rows
                                         instead of 4-byte words at scattered columns (1.80 -> 0.9 ms at N = 2^20 uniform points) */
#define NESVOR_LAYOUT_MASK 3          /* the layout proper; the other bits are hints */
/* `stages` of the owner-computes backward, OR-ed */
#define NESVOR_HG_STAGE_AGGREGATE 1    /* the aggregation launch */
#define NESVOR_HG_STAGE_OWNER 2        /* the owner launch (AGGREGATE then OWNER on one stream == both at once, NESVOR_HG_STAGE_ALL) */
#define NESVOR_HG_STAGE_ALL 3
#define NESVOR_HG_STAGE_KEEP 4         /* a later launch of a split backward (same u, N, workspace): the first launch's queue tails,
                                          sample order and re-ordered dpe are kept */
#define NESVOR_HG_STAGE_ACCUMULATE_U 8 /* the input gradient of this launch's levels is added to grad_u, not written over it */

/* u (N,3) in [0,1]; table flat fp32; pe out. */
int nesvor_hashgrid_forward(const nesvor_grid_t* grid, const float* u, const float* table, float* pe,
                            int64_t N, int layout, void* stream);
/* The same forward; additionally raises the slotted bound pe_absmax (NESVOR_ABSMAX_FLOATS floats, zero-filled by the caller; may
 * be NULL) to max |pe| - the input bound of the network that consumes pe (nesvor_mlp_t.prep + NESVOR_MLP_PREP_XB). */
int nesvor_hashgrid_forward_bounded(const nesvor_grid_t* grid, const float* u, const float* table, float* pe,
                                    int64_t N, int layout, float* pe_absmax, void* stream);
/* The forward for a batch whose consecutive points are NOT spatially clustered (uniform points, a shuffled batch, one point per
 * voxel: the reference's `--no-output-psf` inference, nesvor/nesvor/sample.py:17-33 -> models.py:154-174, and any tcnn-style
 * caller, models.py:25).  `layout` carries NESVOR_LAYOUT_UNCLUSTERED; the points are first put into the order of a coarse
 * lattice's cells (the counting sort of the unclustered backward: three small launches), the one-workgroup-per-256-points kernel
 * runs on workgroups of neighbouring points (lattice boxes in LDS up to the middle levels instead of 8 gathers per point and
 * level), and - feature-major output - the encoded rows are re-ordered into columns by one more launch.  Results are identical to
 * nesvor_hashgrid_forward's (same arithmetic per point).  `workspace`: nesvor_hashgrid_forward_workspace_bytes(grid, N, layout)
 * bytes of scratch (0 without the hint); N < 2^32.  The rows -> columns launch keeps 256 rows of n_levels * n_features + 1 floats
 * in LDS: where that (plus 1 KiB) exceeds the device's LDS per workgroup (n_levels * n_features >= 159 on gfx950) the size query
 * returns -1 for feature-major output and the launch is refused with hipErrorInvalidValue: call nesvor_hashgrid_forward. */
int64_t nesvor_hashgrid_forward_workspace_bytes(const nesvor_grid_t* grid, int64_t N, int layout);
int nesvor_hashgrid_forward_unclustered(const nesvor_grid_t* grid, const float* u, const float* table, float* pe, int64_t N,
                                        int layout, float* pe_absmax, void* workspace, int64_t workspace_bytes, void* stream);
/* The backward: grad_table is ACCUMULATED into (the caller zero-fills when needed); grad_u (N,3) is OVERWRITTEN, or NULL to skip
 * the input gradient.  Owner-computes scatter: LDS aggregation per 256 samples -> per-chunk queues -> one owner workgroup per
 * table chunk.  It is ONE call with five entry points; each names the fields it sets, the others keep their defaults:
 *   nesvor_hashgrid_backward           the common arguments; `stages` bits other than AGGREGATE and OWNER are ignored
 *   nesvor_hashgrid_backward_levels    + level_begin, level_end
 *   nesvor_hashgrid_backward_bounded   + level_begin, level_end, dy_bound
 *   nesvor_hashgrid_backward_plan      + level_begin, level_end, dy_bound, order, cloud_plan
 *   nesvor_hashgrid_backward_adamw     + dy_bound, exp_avg, exp_avg_sq, adam (declared below); KEEP, ACCUMULATE_U and N <= 0 are refused
 * The fields:
 *   workspace    scratch device memory of nesvor_hashgrid_backward_workspace_bytes(grid, N, queue_scale) bytes, shared by the
 *                launches of one backward.  _ex: the same for launches with this `layout` (hints included) - without the point
 *                order's scratch unless NESVOR_LAYOUT_UNCLUSTERED, with room for dpe as rows for NESVOR_LAYOUT_FEATURE_MAJOR |
 *                _UNCLUSTERED | _DY_SCRATCH (not where such rows exceed the copy kernel's LDS, see the forward's query: dpe is then
 *                read in place).  Its first nesvor_hashgrid_backward_workspace_zero_bytes() bytes are zero-filled ONCE after
 *                allocation; the backward keeps them consistent (every aggregation pass zero-fills the next backward's queue tails).
 *   stages       NESVOR_HG_STAGE_*: ALL, or AGGREGATE and OWNER in two calls (to bracket each launch with events, or on two streams).
 *   level_begin, level_end   only these levels (default: all): a data-parallel step runs the fine levels first, starts their
 *                all-reduce and overlaps it with the rest - every launch after the first with KEEP | ACCUMULATE_U.
 *   queue_scale  HOST array of one float per level in (0, 1], or NULL (= 1): the fraction of the worst-case queue capacity (8
 *                records per point and level) to provide.  A record that finds its queue full is added with a global atomic -
 *                exact for any scale - and counted: 32 uint32 counters (one per level) of the latest backward sit at byte
 *                nesvor_hashgrid_backward_overflow_offset(workspace) of the workspace, so a caller can start small (a PSF-cloud batch
 *                fills a few percent) and grow the levels that overflow.  The same array goes to the size query and every launch.
 *   dy_bound     device scalar >= max |dpe| over the batch (any upper bound within ~2^20 of the true maximum keeps fp32
 *                accuracy: the merge table sums in 64-bit fixed point scaled by it), or NULL (default): the kernel determines
 *                each workgroup's maximum itself by reading dpe once more (134 MB at N = 2^20).
 *   order, cloud_plan   the hand-over from the forward of the SAME points, or NULL (default).  The aggregation pass starts with
 *                work that depends on u alone: every 256-point cloud's order by the Morton code of its finest-level cells, its
 *                bounding box, lattice boxes, window bits and box-round schedule.  nesvor_hashgrid_forward_plan is
 *                nesvor_hashgrid_forward_bounded on clustered points (always the per-cloud kernel; pe, pe_absmax bit-identical)
 *                that also writes `order` - nesvor_hashgrid_cloud_order_bytes(N) bytes, exactly those the aggregation pass finds
 *                for itself and keeps at byte nesvor_hashgrid_backward_order_offset() of its workspace - and, unless NULL,
 *                `cloud_plan`: nesvor_hashgrid_cloud_plan_bytes(grid, N) bytes, 16-byte aligned (n_features <= 2; 0 = no plan
 *                for this grid), with the chunking of `queue_scale`.  With `order` no launch sorts, any level range; with
 *                `cloud_plan` too (needs `order`, all levels) the set-up is read from the records.  Both hold for the u, N, grid
 *                and queue_scale they were written for; not with NESVOR_LAYOUT_UNCLUSTERED.
 * N <= 0 returns 0 at once.  hipErrorInvalidValue: n_levels outside 1..32, n_features not 1, 2, 4 or 8, an unknown layout, a NULL
 * workspace, `stages` without a launch, an empty or outside level range, a hand-over against the rules above, and a grid
 * outside the plan's limits (the size queries return -1: use nesvor_hashgrid_backward_atomic) - at most 256 chunks per level (a
 * chunk is the largest power of two of entries with chunk * n_features <= 8192 floats), at most 4064 chunks over all levels, a
 * level's queues below 2^32 bytes and all queues below 2^32 records (8 N records per level at queue_scale 1);
 * nesvor_hashgrid_forward_plan with a cloud_plan refuses such a grid too. */
int64_t nesvor_hashgrid_backward_workspace_bytes(const nesvor_grid_t* grid, int64_t N, const float* queue_scale);
int64_t nesvor_hashgrid_backward_workspace_bytes_ex(const nesvor_grid_t* grid, int64_t N, const float* queue_scale, int layout);
int64_t nesvor_hashgrid_backward_workspace_zero_bytes(void);
int64_t nesvor_hashgrid_backward_overflow_offset(void* workspace);
int64_t nesvor_hashgrid_backward_order_offset(const nesvor_grid_t* grid, int64_t N, const float* queue_scale);
int64_t nesvor_hashgrid_cloud_order_bytes(int64_t N);
int64_t nesvor_hashgrid_cloud_plan_bytes(const nesvor_grid_t* grid, int64_t N);
int nesvor_hashgrid_forward_plan(const nesvor_grid_t* grid, const float* u, const float* table, float* pe, int64_t N, int layout,
                                 float* pe_absmax, void* order, void* cloud_plan, const float* queue_scale, void* stream);
int nesvor_hashgrid_backward(const nesvor_grid_t* grid, const float* u, const float* table, const float* dpe,
                             float* grad_table, float* grad_u, int64_t N, int layout, void* workspace, int stages,
                             const float* queue_scale, void* stream);
int nesvor_hashgrid_backward_levels(const nesvor_grid_t* grid, const float* u, const float* table, const float* dpe,
                                    float* grad_table, float* grad_u, int64_t N, int layout, void* workspace, int stages,
                                    int level_begin, int level_end, const float* queue_scale, void* stream);
int nesvor_hashgrid_backward_bounded(const nesvor_grid_t* grid, const float* u, const float* table, const float* dpe,
                                     float* grad_table, float* grad_u, int64_t N, int layout, void* workspace, int stages,
                                     int level_begin, int level_end, const float* queue_scale, const float* dy_bound,
                                     void* stream);
int nesvor_hashgrid_backward_plan(const nesvor_grid_t* grid, const float* u, const float* table, const float* dpe,
                                  float* grad_table, float* grad_u, int64_t N, int layout, void* workspace, int stages,
                                  int level_begin, int level_end, const float* queue_scale, const float* dy_bound,
                                  const void* order, const void* cloud_plan, void* stream);
/* Same contract, tcnn-style per-corner global atomics (slow on MI355X: memory-side atomics); no workspace, no plan limits. */
int nesvor_hashgrid_backward_atomic(const nesvor_grid_t* grid, const float* u, const float* table, const float* dpe,
                                    float* grad_table, float* grad_u, int64_t N, int layout, void* stream);

/* ------------------------------------------------------------------------
 * PSF sampling + rigid transform of a batch of slice pixels.  Replaces the head of
 * NeSVoR.forward (nesvor/nesvor/models.py:267-278), ax/mat_transform_points
 * (nesvor/transform/transform.py:259-280, trans_first = True) and the bounding-box
 * normalisation of INR.forward (models.py:143):
 *   x[b,s] = R_k (xyz[b] + noise[b,s] * sigma_k + t_k),  k = slice_idx[b];  u = (x - bb0)/(bb1 - bb0)
 * mat (n,3,4) per-slice [R|t]; slice_idx (B) int64; xyz (B,3); sigma (n,3); noise (B,S,3)
 * standard normal; bb (2,3); x (B,S,3) out; u (B*S,3) out or NULL.
 * backward: dx (B,S,3) and/or du (B*S,3) (either may be NULL) -> dmat (B,3,4) per PIXEL
 * (gradient w.r.t. the pixel's slice matrix; the caller index-adds pixels into slices).
 * ---------------------------------------------------------------------- */
int nesvor_psf_transform_forward(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                 const float* noise, const float* bb, float* x, float* u, int B, int S, void* stream);
int nesvor_psf_transform_backward(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                  const float* noise, const float* bb, const float* dx, const float* du, float* dmat,
                                  int B, int S, void* stream);
/* The same two operators with the PSF noise drawn inside the kernels: xi[b,s] = the three N(0,1) draws of a counter-based
 * generator (Philox4x32-10) keyed by `seed`, counter = (sample index b*S+s, `offset`) - nothing is stored, the backward
 * evaluates the same function.  The reference draws torch.randn (models.py:270); any N(0,1) stream is the same model.
 * x (and u) may be NULL when not needed.  nesvor_psf_noise writes the draws themselves, (n_samples, 3). */
int nesvor_psf_transform_forward_rng(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                     uint64_t seed, uint64_t offset, const float* bb, float* x, float* u, int B, int S,
                                     void* stream);
/* The same launch also gathers se[b, :] = embedding[slice_idx[b], :] ((B, ks); ks = 0: nothing) - the per-pixel input of
 * sigma_net / b_net of the training step (the `slice_embedding(slice_idx)` lookup of nesvor/nesvor/models.py:281). */
int nesvor_psf_transform_forward_rng_gather(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                            uint64_t seed, uint64_t offset, const float* bb, float* x, float* u, int B, int S,
                                            const float* embedding, float* se, int ks, void* stream);
int nesvor_psf_transform_backward_rng(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                      uint64_t seed, uint64_t offset, const float* bb, const float* dx, const float* du,
                                      float* dmat, int B, int S, void* stream);
/* The same backward; every pixel's gradient is also (dpix non-NULL) or only (dpix NULL) ADDED to row slice_idx[b] of dmat_slice
 * (n,3,4) - the caller zero-fills it -, i.e. the index_add over slice_idx the reference's autograd performs, without a second
 * launch over dpix. */
int nesvor_psf_transform_backward_rng_slices(const float* mat, const int64_t* slice_idx, const float* xyz, const float* sigma,
                                             uint64_t seed, uint64_t offset, const float* bounding_box, const float* dx,
                                             const float* du, float* dpix, float* dmat_slice, int B, int S, void* stream);
int nesvor_psf_noise(uint64_t seed, uint64_t offset, float* out, int64_t n_samples, void* stream);

/* ------------------------------------------------------------------------
 * Fused small MLP (fp32 matrix cores).  Replaces the nn.Linear/ReLU stacks that
 * build_network creates in single-precision mode (nesvor/nesvor/models.py:42-67)
 * for density_net (:113-121), sigma_net (:238-246) and b_net (:249-258), plus the
 * expand/cat glue of NeSVoR.net_forward (:339-353).
 *   input  = [ xa[n / samples_per_pixel][0..k_a) | xb[b_row0 .. b_row0+k_b)[n] ]
 *            xa: (P, k_a) per-pixel features or NULL (k_a = 0); xb: (rows, N) feature-major
 *   layers = Linear(k_a+k_b, 64) ReLU [Linear(64,64) ReLU]*(n_hidden-1) Linear(64, out_dim)
 *            weight[l]: (out,in) row-major as in nn.Linear; bias[l]: (out)
 *   y      : (out_dim, N) feature-major
 * saved_hidden[l] (l < n_hidden): N_pad16*64 floats each, written by forward (pass
 * NULL for inference), read by backward.  dpre_scratch[l]: same size, scratch.
 * backward: dy (out_dim,N) -> dxa (N,k_a) per-sample (or NULL), dxb (k_b,N) (or NULL)
 * and dw_partial (n_partial, sum_l(out*in+out)) partial parameter gradients in
 * order W0,b0,W1,b1,.. that the caller sums over dim 0 (no atomics anywhere).
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t width;              /* hidden width; 64.  LIMIT: the fused kernels are built around one 64-column tile per layer (four
                                 16-feature blocks, weights resident in LDS as MFMA operand images).  The reference takes any
                                 --width / --depth (nesvor/cli/main.py:68-73, build_network models.py:42-67): widths below 64
                                 run zero-padded on these kernels (exactly the same function; nesvor_amd/mlp.py::kernel_params),
                                 depth up to NESVOR_MAX_MLP_LAYERS - 1 hidden layers is native, and anything wider or deeper is
                                 REFUSED here (hipErrorInvalidValue) and taken by nesvor_mlp_wide_t below (round 6: width <= 128,
                                 up to seven hidden layers, hand-written fp32-MFMA kernels; rounds 3-5 evaluated those shapes
                                 with rocBLAS under autograd).  tests/test_gpu_parity.py::test_other_widths_and_depths_match_oracle_losses
                                 holds 128 x 1, 64 x 4 and 96 x 5 to the oracle.  Only beyond THOSE limits does the host side
                                 (nesvor_amd/mlp.py::library_mlp) fall back to library GEMMs */
  int32_t n_hidden;           /* hidden layers, 1..NESVOR_MAX_MLP_LAYERS-1 */
  int32_t out_dim;            /* 1..16 */
  int32_t k_a, k_b, b_row0;
  int32_t samples_per_pixel;
  int32_t dxa_group_sums;     /* backward only: dxa is (N/16, k_a), one row per 16-sample group = the sum over its samples
                                 (needs N, samples_per_pixel and k_a multiples of 16 and the fused backward) */
  int32_t bf16_operands;      /* how the matrix products are evaluated (storage, accumulation, outputs are fp32 in all modes):
                                 0: fp32 MFMA (v_mfma_f32_16x16x4_f32, an fp32 FMA chain);
                                 1: operands (weights, activations, upstream gradients) rounded to bf16 - an opt-in
                                    mixed-precision mode, not the reference's fp32 semantics; the saved activations
                                    are bf16.  Backward: wave-specialised kernel only (N, S, k_a multiples of 16, at
                                    most two hidden layers, k_a + k_b <= 32 for two hidden layers);
                                 2: every fp32 operand x written as two fp16 numbers of a scaled copy (x s = hi + lo, both
                                    roundings to nearest, s a power of two per operand tensor and launch derived from the
                                    bounds in `prep`), three fp16 MFMAs per product, fp32 accumulation: fp32-equivalent accuracy
                                    (error against fp64 at or below the fp32 FMA chain's: tools/f16_split_probe.hip,
                                    tests/test_gpu_ops.py::test_fused_mlp_split_operands_keep_fp32_accuracy) on the 16x
                                    faster 16-bit matrix pipe.  Pipelined forward and wave-specialised backward (dX chain and dW
                                    products); every other kernel evaluates this mode as mode 0, which is always a valid
                                    evaluation of it.  (Rounds 2-4: three bf16 terms per operand, six MFMAs per product.)
                                    One quantity is NOT at the fp32 chain's error: the bias gradients of the HIDDEN layers.
                                    MEASURED: every entry of db comes out too small, at N = 2^18 by -1.2e-6 .. -1.9e-6 of
                                    max |db| on average, 1.9e-6 .. 5.2e-6 at most, against +-1e-7 .. 2e-7 in mode 0 (2^14:
                                    8e-7 .. 1.3e-6), while dX and dW are at the fp32 chain's error;
                                    tests/test_gpu_mlp_steady_state.py prints it per case.  NOT ESTABLISHED: the cause.  A
                                    one-signed error of each pre-activation gradient (~2^-26 of its size, as from 16-bit-MFMA
                                    accumulators that are not rounded to nearest) would fit - harmless where signs mix, adding
                                    up like N in db = sum over the batch of dpre against a sum that grows like sqrt(N) - but
                                    nothing has isolated it.
                                    REQUIRES `prep`;
                                 3: operands rounded to fp16 (the reference's default arithmetic; overflows beyond 65504: its
                                    GradScaler's job), same kernels as mode 1;
                                 4: "scaled fp16" (round 6): mode 2's scales, operand images, bits-only save and per-sample
                                    backward scale with the LEADING term of every split alone - operands rounded to fp16 after
                                    scaling (no overflow, no loss scaler), ONE MFMA per product in the pipelined forward and the
                                    compact wave-specialised backward; every other kernel evaluates it as mode 2 or mode 0 (more
                                    accurate, always valid).  REQUIRES `prep`.  The only mode that takes a bias-free network (NULL
                                    `bias`, see there: the half-precision model structure).  Measured: DESIGN.md section 4. */
  int32_t compact_save;       /* 1: training keeps, per hidden unit and sample, ONE BIT (h > 0) of every hidden layer and nothing
                                 else: saved_hidden[0] = one uint32 per (16-sample group, lane) - 16 N bytes instead of 256 N
                                 per hidden layer - with bit 16 l + 4 b + r = [pre-activation sign bit clear] (= [h_l > 0] for every
                                 value but an exact +0: the gate then passes a gradient the reference's ReLU'(0) = 0 drops - the
                                 convention of this mode, see tests/test_gpu_ops.py::test_fused_mlp_compact_save) for the unit the
                                 lane holds in block b, element r of the fragment layout; saved_hidden[l >= 1] are not
                                 touched (any non-NULL pointer).  The backward gates with the bits and RECOMPUTES every hidden
                                 layer from the network input (the forward's own products, 12 + 24 MFMAs per 16 samples at two
                                 hidden layers) instead of streaming it back: 536 MB less written and 670 MB less read per
                                 network and step at N = 2^20.  (Rounds 3-4 kept the values of the layers after the first.)
                                 Needs what nesvor_mlp_compact_save_ok() checks (split operands, the pipelined forward and
                                 the wave-specialised backward); forward and backward of one step must agree on it. */
  const float* weight[NESVOR_MAX_MLP_LAYERS];
  const float* bias[NESVOR_MAX_MLP_LAYERS];  /* (out), or ALL NULL: a bias-free network (tinycudann's half-precision structure) -
                                 bf16_operands = 4 only.  It runs the pipelined forward and the compact wave-specialised backward
                                 in their bias-free forms (no bias loads, no bias-gradient sums) and, for every other case (a full save,
                                 shapes those kernels refuse), the wide kernels below, which evaluate a NULL bias as zero.  Its
                                 dw_partial rows have NO b columns: W0 | W1 | ... | W_last (out_dim rows), a prefix of tinycudann's
                                 flat parameter layout.  A NULL bias in any other mode, or next to non-NULL biases, is refused
                                 (hipErrorInvalidValue) by every entry point; a descriptor without weight pointers (a shape query)
                                 counts as biased.  Weight norms take max |b| = 0 for a NULL bias. */
  const float* prep;          /* mode 2: NESVOR_MLP_PREP_FLOATS device floats, valid bounds for THIS launch (a bound may be loose -
                                 it costs resolution below 2^-17 of it - but never too small: fp16 overflows at 65504 s).
                                 Operand bounds are SLOTTED: NESVOR_ABSMAX_FLOATS floats each, the bound is the maximum of every
                                 NESVOR_ABSMAX_STRIDE-th of them
                                 (publishing kernels spread their atomic maxima over the slots by workgroup):
                                   [NESVOR_MLP_PREP_XA ..] >= max |xa|, [NESVOR_MLP_PREP_XB ..] >= max |xb rows b_row0 .. b_row0 + k_b|,
                                   [NESVOR_MLP_PREP_DY ..] >= max |dy| (backward),
                                   [NESVOR_MLP_PREP_LAYER0 + 4 l + {0,1,2,3}] = max |W_l|, max_o sum_k |W_l[o][k]|,
                                   max_k sum_o |W_l[o][k]|, max |b_l|.
                                 nesvor_mlp_prepare() fills any part of it; inside the training step the producing kernels publish
                                 the operand bounds (hash-grid forward: max |pe|; the networks' y_absmax / dxb_absmax; the loss
                                 kernel: max |d z|, max |d log_var|) and one launch per step takes the weight norms.  Forward
                                 and backward of one step must see the same [0], [1] and weights. */
  float* y_absmax;            /* forward, optional: a slotted bound (NESVOR_ABSMAX_FLOATS zero-filled device floats) raised to max |y| */
  const void* weight_images;  /* mode 2, optional (NULL: every launch builds its LDS operand images from `weight`, as rounds 2-5 did):
                                 nesvor_mlp_weight_images_bytes(net) device bytes holding the split fp16 operand images of ALL layers
                                 for the CURRENT weights - written by nesvor_mlp_prepare_weights_images() together with the weight
                                 norms, so that the images' scales are the ones `prep` yields.  The training step (csrc/step.hip)
                                 builds them once per iteration for its four MLP launches (round 6; measured: -3.4 us of a 0.284 ms
                                 step at 2^17 points, within noise at 2^20).  Bit-identical to the in-kernel builds
                                 (tests/test_gpu_ops.py::test_fused_mlp_prebuilt_weight_images_are_bit_identical). */
} nesvor_mlp_t;
/* nesvor_mlp_t.bf16_operands, as documented at the field */
#define NESVOR_MLP_MODE_FP32 0
#define NESVOR_MLP_MODE_BF16 1
#define NESVOR_MLP_MODE_SPLIT 2
#define NESVOR_MLP_MODE_FP16 3
#define NESVOR_MLP_MODE_FP16_SCALED 4
#define NESVOR_ABSMAX_SLOTS 16      /* a slotted bound: this many floats, NESVOR_ABSMAX_STRIDE floats (one 256-byte line) apart - */
#define NESVOR_ABSMAX_STRIDE 64     /* atomics on one cache line serialise at the memory side, publishers spread by workgroup */
#define NESVOR_ABSMAX_FLOATS (NESVOR_ABSMAX_SLOTS * NESVOR_ABSMAX_STRIDE)
#define NESVOR_MLP_PREP_XA 0
#define NESVOR_MLP_PREP_XB (1 * NESVOR_ABSMAX_FLOATS)
#define NESVOR_MLP_PREP_DY (2 * NESVOR_ABSMAX_FLOATS)
#define NESVOR_MLP_PREP_LAYER0 (3 * NESVOR_ABSMAX_FLOATS)
#define NESVOR_MLP_PREP_FLOATS (NESVOR_MLP_PREP_LAYER0 + 4 * NESVOR_MAX_MLP_LAYERS)
#define NESVOR_MLP_WHAT_INPUT 1   /* `what` of nesvor_mlp_prepare: the xa and xb bounds */
#define NESVOR_MLP_WHAT_DY 2      /* the dy bound */
#define NESVOR_MLP_WHAT_WEIGHTS 4 /* the per-layer norms from net->weight / net->bias */
/* Fill (parts of) `prep` for `net` on `stream`: absolute maxima by a grid-wide reduction (the selected entries are zero-filled
 * first), weight norms by one workgroup per layer.  xa / xb / dy may be NULL when their bit is not set. */
int nesvor_mlp_prepare(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy, int64_t N, float* prep,
                       int what, void* stream);
/* The weight norms of up to three networks in ONE launch (the training step: once per iteration, on its side stream);
 * optionally also max |x[0..n_x)| into the slotted bound `x_slots` (the slice embedding table: the pixel features of
 * sigma_net / b_net are rows of it).  preps[i] as nesvor_mlp_t.prep of nets[i]; nothing is zero-filled. */
int nesvor_mlp_prepare_weights(const nesvor_mlp_t* const* nets, float* const* preps, int n_nets, const float* x, int64_t n_x,
                               float* x_slots, void* stream);

/* ... the same launch also writing each network's split operand images (nesvor_mlp_t.weight_images): images[i] = NULL or
 * nesvor_mlp_weight_images_bytes(nets[i]) device bytes (16-byte aligned); `images` itself may be NULL. */
int nesvor_mlp_prepare_weights_images(const nesvor_mlp_t* const* nets, float* const* preps, void* const* images, int n_nets,
                                      const float* x, int64_t n_x, float* x_slots, void* stream);
/* Size of a network's prebuilt operand images (0: a shape the split-mode kernels do not take). */
int64_t nesvor_mlp_weight_images_bytes(const nesvor_mlp_t* net);

/* 1 if (net, N) can run with compact_save = 1 (the field itself is ignored by this query), else 0. */
int nesvor_mlp_compact_save_ok(const nesvor_mlp_t* net, int64_t N);
/* 1 if `net` (weight pointers set, bf16_operands = 4; its bias pointers are ignored) runs forward and backward with NULL biases on
 * hand-written kernels at N, else 0.  The backward of a bias-free network is fused (nesvor_mlp_backward_fused_ok) exactly when its
 * training forward saves compactly (nesvor_mlp_compact_save_ok); otherwise it runs the wide dX + dW pair through dpre scratch. */
int nesvor_mlp_bias_free_ok(const nesvor_mlp_t* net, int64_t N);

int nesvor_mlp_forward(const nesvor_mlp_t* net, const float* xa, const float* xb, float* y,
                       float* const* saved_hidden, int64_t N, void* stream);
/* 1 if (net, N) is a shape the fused backward takes - dX, dW and db in ONE wave-specialised launch, no dpre scratch (pass NULL
 * entries): N, samples_per_pixel and k_a multiples of 16, at most two hidden layers, at most two 16-row input blocks at two
 * hidden layers.  GUARANTEE: an answer of 1 implies N % 16 == 0, samples_per_pixel % 16 == 0 and k_a % 16 == 0 - every 16-sample
 * group lies inside one pixel - so 1 is also the rule for who may ask for per-group pixel-feature gradients (dxa_group_sums);
 * callers do not repeat the divisibility test.  The converse does not hold (a divisible shape may be refused).
 * 0: pass dpre_scratch[l] (N_pad16 * 64 floats each) and the backward runs as a dX launch + a dW launch: on fp32
 * MFMAs for bf16_operands = 0 / 2 / 4 (nesvor_mlp_wide_backward_bounded), on 16-bit operands rounded at the fused kernel's points for
 * bf16_operands = 1 / 3 (any shape the 16-bit forward takes; dxa per sample, dxa_group_sums = 0). */
int nesvor_mlp_backward_fused_ok(const nesvor_mlp_t* net, int64_t N);
int nesvor_mlp_backward(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy,
                        float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb,
                        float* dw_partial, int n_partial, int64_t N, void* stream);
/* The same backward; additionally raises the device scalar *dxb_absmax (atomic max; the caller zero-fills it) to max |dxb|
 * when dxb_absmax and dxb are non-NULL: the consumer of dxb - the hash-grid backward, nesvor_hashgrid_backward_bounded -
 * then needs no pass of its own over the gradient to scale its fixed-point sums. */
int nesvor_mlp_backward_bounded(const nesvor_mlp_t* net, const float* xa, const float* xb, const float* dy,
                                float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb,
                                float* dw_partial, int n_partial, int64_t N, float* dxb_absmax, void* stream);

/* ------------------------------------------------------------------------
 * The same networks at ANY width up to 256 and up to NESVOR_MLP_WIDE_MAX_LAYERS - 1 hidden layers (round 6; csrc/mlp_wide.hip):
 * the reference builds its MLPs with any --width / --depth (nesvor/cli/main.py:68-73 -> build_network,
 * nesvor/nesvor/models.py:42-67; bias-free tinycudann.Network in half precision, models.py:28-41), and shapes outside
 * nesvor_mlp_t's (width 64, at most three hidden layers) used to leave the hand-written path for library GEMMs.  fp32 matrix
 * cores (v_mfma_f32_16x16x4_f32: an fp32 FMA chain), activations in registers from input to output, ONE layer's weights in LDS
 * at a time (a 128 x 128 layer is 64 KB: the workgroup swaps the operand image between layers of a 256-sample tile).  Above
 * width 128 a layer's image (256 KB at width 256) exceeds the CU's 160 KiB of LDS: it streams through LDS as a CHUNKED image,
 * 32 output rows x all k at a time in two alternating 32 KB buffers (one barrier per chunk, the next chunk's loads in flight
 * behind this chunk's MFMAs), under 128-sample tiles of one 16-sample group per wave; the saved / dpre fragments have sixteen
 * blocks per group (nesvor_mlp_wide_saved_floats = N padded to 16, times 256), of which the blocks at or beyond
 * ceil(width / 16) are padding that no kernel writes or reads.
 * Widths that are not multiples of 16 run zero-padded (exactly the same function).  Input composition, layouts and the meaning of
 * xa / xb / b_row0 / k_a / k_b / samples_per_pixel as for nesvor_mlp_t; k_a + k_b <= 64, out_dim <= 16.
 *   forward : y (out_dim, N); saved_hidden = n_hidden device buffers of nesvor_mlp_wide_saved_floats(net, N) floats each (the
 *             post-ReLU activations in MFMA fragment layout) or NULL (inference);
 *   backward: dy (out_dim, N) -> dxa (N, k_a) per SAMPLE (or NULL), dxb (k_b, N) (or NULL), dw_partial (n_partial,
 *             nesvor_mlp_wide_param_count(net)): per-workgroup partial sums in nn.Linear parameter order W0, b0, W1, b1, ...
 *             (no b columns for a NULL bias), to be summed over the rows by the caller; dpre_scratch = n_hidden buffers of the
 *             saved buffers' size.  Two launches (dX chain, then dW / db), no atomics.
 * Errors: hipErrorInvalidValue for shapes outside the limits (a width beyond 256 included: nesvor_mlp_wide_param_count returns
 * -1 for them) or missing buffers. */
#define NESVOR_MLP_WIDE_MAX_LAYERS 8
typedef struct {
  int32_t width;              /* hidden width, 1..256 */
  int32_t n_hidden;           /* 1..NESVOR_MLP_WIDE_MAX_LAYERS-1 */
  int32_t out_dim;            /* 1..16 */
  int32_t k_a, k_b, b_row0;
  int32_t samples_per_pixel;
  int32_t reserved;
  const float* weight[NESVOR_MLP_WIDE_MAX_LAYERS];  /* nn.Linear layout (out, in), fp32 */
  const float* bias[NESVOR_MLP_WIDE_MAX_LAYERS];    /* (out) or NULL: bias-free layer */
} nesvor_mlp_wide_t;
int64_t nesvor_mlp_wide_saved_floats(const nesvor_mlp_wide_t* net, int64_t N);
int nesvor_mlp_wide_param_count(const nesvor_mlp_wide_t* net);
int nesvor_mlp_wide_forward(const nesvor_mlp_wide_t* net, const float* xa, const float* xb, float* y, float* const* saved_hidden,
                            int64_t N, void* stream);
int nesvor_mlp_wide_backward(const nesvor_mlp_wide_t* net, const float* xa, const float* xb, const float* dy,
                             float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb, float* dw_partial,
                             int n_partial, int64_t N, void* stream);
/* ... additionally raising the device scalar *dxb_absmax to max |dxb| (as nesvor_mlp_backward_bounded does; NULL: not wanted).  At
 * width 64 the saved / dpre buffers have the fragment layout of nesvor_mlp_t's full save: nesvor_mlp_backward_bounded hands the
 * shapes its wave-specialised kernel does not take (ragged N, samples per pixel or pixel features not in multiples of 16, three
 * hidden layers) to this entry point in the fp32 modes (0, 2, 4); the 16-bit operand modes (1, 3) run mlp.hip's 16-bit launch pair. */
int nesvor_mlp_wide_backward_bounded(const nesvor_mlp_wide_t* net, const float* xa, const float* xb, const float* dy,
                                     float* const* saved_hidden, float* const* dpre_scratch, float* dxa, float* dxb,
                                     float* dw_partial, int n_partial, int64_t N, float* dxb_absmax, void* stream);

/* ------------------------------------------------------------------------
 * Imaging model + losses, value and gradient in one launch.  Replaces the tail of
 * NeSVoR.forward (nesvor/nesvor/models.py:286-325), edge_reg/tv_reg/l2_reg
 * (models.py:366-384) and their autograd backward.  See csrc/loss.hip for the math.
 * Inputs (device): z0, log_var, log_bias (B*S) [log_var / log_bias may be NULL],
 * x (B,S,3), v (B), slice_idx (B) int64, c (n) slice scale or NULL, log_var_slice (n) or
 * NULL, log_bias_mean (1) (only read when log_bias != NULL).
 * Forward launch (gw == NULL) writes loss_pix (B,3) = per-pixel [MSE term, logVar term,
 * sum_s regulariser term].  Backward launch (gw = device pointer to the 4 upstream
 * gradients d total / d {MSE, logVar, imageReg, biasReg}) writes dz0, dlog_var, dlog_bias
 * (B*S), dx (B,S,3) or NULL, dc_pix (B) or NULL, dlvs_pix (B) or NULL; if loss_pix is
 * non-NULL as well, the same launch also writes the loss values.
 * reg_type: 0 edge, 1 TV, 2 L2.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* z0; const float* log_var; const float* log_bias; const float* x; const float* v;
  const int64_t* slice_idx; const float* c; const float* log_var_slice; const float* log_bias_mean;
  const float* gw;
  float* loss_pix; float* dz0; float* dlog_var; float* dlog_bias; float* dx; float* dc_pix; float* dlvs_pix;
  int32_t B, S, reg_type;
  float delta;
  /* optional (backward launch): slotted bounds (NESVOR_ABSMAX_FLOATS floats each, zero-filled by the caller) raised to max |dz0|,
     max |dlog_var|, max |dlog_bias| - the upstream-gradient bounds of the networks that consume them
     (nesvor_mlp_t.prep + NESVOR_MLP_PREP_DY) */
  float* dz0_absmax; float* dlog_var_absmax; float* dlog_bias_absmax;
} nesvor_loss_t;

int nesvor_imaging_loss(const nesvor_loss_t* args, void* stream);

/* Per-pixel -> per-slice gradient accumulation of one training iteration (the index_add /
 * embedding-backward / sum-over-samples steps autograd runs for models.py:267-325):
 *   dc[k] += dc_pix[b]; dlvs[k] += dlvs_pix[b]; dmat[k,:] += dpix[b,:] (12 floats);
 *   dse[k,:] += sum_s dxa[b,s,:]   with k = slice_idx[b].
 * dxa (B*S, ks) per-sample gradient w.r.t. the slice embedding fed to an MLP.  Any of the four
 * source pointers may be NULL (skipped).  Outputs are ACCUMULATED into (caller zero-fills). */
/* Small-tensor bookkeeping of one training iteration (nesvor_amd/direct.py), one launch each:
 *   prologue: c (n) = n softmax(logit_coef) (models.py:296; logit_coef may be NULL), mat (n,3,4) =
 *             axisangle2mat(axisangle) (axisangle may be NULL), zero_buf[0..n_zero) = 0;
 *   epilogue: dlogit (n) = c (dc - <dc,c>/n) (dc may be NULL); daxisangle (n,6) = axisangle2mat_backward(dmat,
 *             axisangle) + w_trans * dtrans and losses[3] = sum(trans_terms) (dmat may be NULL);
 *             losses[0,1,2,4] = {MSE, logVar, MSE+logVar, imageReg} from loss_pix (B,3) (nesvor_imaging_loss):
 *             imageReg = img_scale * sum(loss_pix[:,2]) + img_offset. */
int nesvor_step_prologue(const float* logit_coef, float* c, const float* axisangle, float* mat, float* zero_buf,
                         int n_zero, int n, void* stream);
/* The same launch with one more workgroup: NeSVoR.trans_loss (nesvor_trans_loss's arithmetic) for the n slices -
 * trans_terms (n) and g_trans (n,6) are overwritten.  axisangle_init NULL: exactly nesvor_step_prologue. */
int nesvor_step_prologue_pose(const float* logit_coef, float* c, const float* axisangle, float* mat, float* zero_buf,
                              int n_zero, int n, const float* axisangle_init, float* trans_terms, float* g_trans, void* stream);
int nesvor_step_epilogue(const float* dc, const float* c, float* dlogit, const float* dmat, const float* axisangle,
                         const float* dtrans, float w_trans, float* daxisangle, const float* loss_pix,
                         const float* trans_terms, float* losses, int n, int B, float img_scale, float img_offset,
                         void* stream);
/* The same launch with the pose regulariser's weight multiplied by a DEVICE float: w_trans * (*w_trans_scale) (the loss scale
 * of nesvor_loss_scaler_t, read by the kernel).  w_trans_scale NULL: exactly nesvor_step_epilogue. */
int nesvor_step_epilogue_scaled(const float* dc, const float* c, float* dlogit, const float* dmat, const float* axisangle,
                                const float* dtrans, float w_trans, const float* w_trans_scale, float* daxisangle,
                                const float* loss_pix, const float* trans_terms, float* losses, int n, int B, float img_scale,
                                float img_offset, void* stream);
int nesvor_slice_grads(const int64_t* slice_idx, const float* dc_pix, const float* dlvs_pix, const float* dxa,
                       const float* dpix, float* dc, float* dlvs, float* dse, float* dmat, int B, int S, int ks,
                       void* stream);
/* The same sums without atomics: one workgroup per slice lists the batch's pixels of its slice (in batch order: reproducible
 * sums) and adds their totals to the outputs it alone owns.  Needs B <= 4096 and 256 % ks == 0 (or dxa == NULL); returns
 * hipErrorInvalidValue (= 1) otherwise, and the caller falls back to nesvor_slice_grads. */
int nesvor_slice_grads_by_slice(const int64_t* slice_idx, const float* dc_pix, const float* dlvs_pix, const float* dxa,
                                const float* dpix, float* dc, float* dlvs, float* dse, float* dmat, int B, int S, int ks,
                                int n_slices, void* stream);

/* ------------------------------------------------------------------------
 * Fused AdamW over a flat fp32 parameter buffer.  Replaces the
 * torch.optim.AdamW step at nesvor/nesvor/train.py:144-152,195-197
 * (betas (0.9,0.99), eps 1e-15, decoupled weight decay):
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 * grad is multiplied by grad_scale first (DDP mean) and, if zero_grad != 0,
 * zero-filled afterwards (fuses optimizer.zero_grad()).
 * ---------------------------------------------------------------------- */
int nesvor_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay,
                      float bias_correction1, float bias_correction2, float grad_scale, int zero_grad,
                      void* stream);

/* The same numbers as one struct (bias_correction{1,2} = 1 - beta{1,2}^t of the step being taken). */
typedef struct {
  float lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, grad_scale;
} nesvor_adamw_t;

/* ------------------------------------------------------------------------
 * Loss scaler on the device (csrc/scaler.hip): torch.cuda.amp.GradScaler as the reference configures it
 * (nesvor/nesvor/train.py:161-164, 190-196) without a host read per iteration.  One struct per trainer, in device
 * memory, 32 bytes; every field is read and written by the kernels below only (the host writes it before a step or
 * reads it after one, on the same stream).
 *   scale:          the loss scale every gradient of the step carries;
 *   growth_factor, backoff_factor, growth_interval: the GradScaler settings;
 *   growth_tracker: finite steps in a row since the last growth / backoff;  skipped: overflowing steps so far;
 *   t:              the optimizer's step count (steps taken; a skipped step does not count);
 *   found_inf:      non-zero once nesvor_grad_found_inf saw a NaN or an Inf since the last nesvor_loss_scaler_update.
 * ---------------------------------------------------------------------- */
typedef struct nesvor_loss_scaler_t {
  float scale, growth_factor, backoff_factor;
  int32_t growth_interval, growth_tracker, skipped, t;
  uint32_t found_inf;
} nesvor_loss_scaler_t;

/* found_inf |= any(!isfinite(grad[0..n))): NaN, +Inf and -Inf count.  Any 4-byte aligned grad. */
int nesvor_grad_found_inf(const float* grad, int64_t n, nesvor_loss_scaler_t* s, void* stream);
/* nesvor_adamw_step predicated on the device state: if s->found_inf is zero, exactly nesvor_adamw_step with
 * bias_correction{1,2} = 1 - beta{1,2}^(s->t + 1) (evaluated in double, as the host does, then rounded to float) and
 * grad_scale = 1 / (world_size * s->scale) (likewise); otherwise param / exp_avg / exp_avg_sq are not touched and grad is
 * zero-filled if zero_grad != 0.  s->t is NOT advanced here (nesvor_loss_scaler_update does).  param, grad, exp_avg and
 * exp_avg_sq 16-byte aligned. */
int nesvor_adamw_step_scaled(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                             double beta2, float eps, float weight_decay, int world_size, int zero_grad,
                             const nesvor_loss_scaler_t* s, void* stream);
/* The scaler's update, one lane (GradScaler.update): a finite step advances t and growth_tracker and multiplies the scale by
 * growth_factor when growth_tracker reaches growth_interval (tracker back to 0); an overflowing step multiplies it by
 * backoff_factor, resets growth_tracker and counts in skipped.  found_inf is cleared. */
int nesvor_loss_scaler_update(nesvor_loss_scaler_t* s, void* stream);
/* out[i] = base[i] * s->scale, i < n: the loss kernel's upstream weights (nesvor_loss_t.gw) under the device scale. */
int nesvor_loss_scale_weights(const float* base, float* out, int n, const nesvor_loss_scaler_t* s, void* stream);

/* Hash-grid backward whose owner pass also takes the AdamW step on the table: the workgroup that completes a chunk's
 * gradient updates table / exp_avg / exp_avg_sq of that chunk while the gradient is still in LDS, so the table gradient
 * never travels through HBM.  Equals nesvor_hashgrid_backward_bounded(stages) over all levels followed by
 * nesvor_adamw_step(table, grad_table, exp_avg, exp_avg_sq, <table numel>, ..., zero_grad = 1): grad_table is read (it may
 * hold an earlier backward's gradient) and is all zero afterwards, but the gradient of THIS backward is never stored in it.
 * One of the entry points of the hash-grid backward's contract (above): stages AGGREGATE, OWNER (+ AdamW) or both, all levels.
 * table, exp_avg, exp_avg_sq, grad_table: (sum of level sizes, F), the layout nesvor_hashgrid_forward reads. */
int nesvor_hashgrid_backward_adamw(const nesvor_grid_t* grid, const float* u, float* table, const float* dpe,
                                   float* grad_table, float* grad_u, int64_t N, int layout, void* workspace, int stages,
                                   const float* queue_scale, const float* dy_bound, float* exp_avg, float* exp_avg_sq,
                                   const nesvor_adamw_t* adam, void* stream);
/* out[c] = sum_r in[r * ld + c], c < cols, for a row-major matrix of row pitch ld >= cols floats: reduces the
 * dw_partial of nesvor_mlp_backward (the `partial.sum(0)` of the host side) straight into a gradient segment; with
 * ld > cols, a column range of it (one layer's weights when the model keeps no biases, tinycudann.Network). */
int nesvor_sum_rows(const float* in, float* out, int rows, int cols, int ld, void* stream);
/* n_jobs <= 4 of those sums (same number of rows) in one launch; in / out / cols / ld: host arrays of n_jobs entries. */
int nesvor_sum_rows_multi(const float* const* in, float* const* out, const int* cols, const int* ld, int n_jobs, int rows,
                          void* stream);

/* ------------------------------------------------------------------------
 * One training iteration behind one entry point (csrc/step.hip).  Replaces the loop body of the reference's train()
 * (nesvor/nesvor/train.py:179-197: NeSVoR.forward models.py:260-327, loss.backward(), optimizer.step(), zero_grad()):
 * the host enqueues every launch of the iteration - sampler, hash grid, MLPs, imaging loss, the backwards, per-slice
 * gradients, AdamW - with one call, into workspace buffers the caller allocated once for (B, S).  All pointers are device
 * pointers unless stated; gradients go straight into the caller's (flat) gradient buffer, which the AdamW step zero-fills.
 *   switches   : opt_T = !no_transformation_optimization, has_lv = !no_pixel_variance, has_c = !no_slice_scale,
 *                has_lvs = !no_slice_variance, has_b = n_levels_bias > 0 (cli/main.py:61,86-110)
 *   small      : n (1 + 12 + 13) + 1 + 3 NESVOR_MLP_PREP_FLOATS floats: slice scale c | pose matrices | zeroed accumulators
 *                [dc | dmat] | max |dpe| | the three networks' operand bounds and weight norms (nesvor_mlp_t.prep; the step
 *                points density / sigma / bias_net at them itself)
 *   saved_*    : per hidden layer N_pad16 * 64 floats (nesvor_mlp_forward; slot 0 of a network with compact_save: 4 N_pad16
 *                floats);  partial: 3 x NESVOR_STEP_MLP_PARTIALS x (largest network's parameter count) floats - one third per
 *                network, summed by one nesvor_sum_rows_multi launch;  losses (run argument): 6 floats {MSE, logVar, MSE+logVar, transReg,
 *                imageReg, biasReg} (models.py:14-19)
 *   queue_scale: HOST array (nesvor_hashgrid_backward);  side_stream: a second stream of the same device (early per-slice
 *                gradients, owner pass of the hash-grid backward); with overlap_owner the table gradient is complete only behind the
 *                side stream - the step joins it itself before its own AdamW, a caller that runs the optimizer makes
 *                its stream wait for side_stream
 * nesvor_step_run(phase = 0): the whole iteration.  Data parallel: phase 1 = everything up to and including the hash-grid
 * backward of levels [split_level, L) (the host then starts the all-reduce of that part of the table gradient), phase 2 =
 * the remaining levels and the rest of the iteration.  adam == NULL: no optimizer step (the caller reduces gradients first).
 * With has_b, phase 0 or phase 1 can itself stop at the bias field's mean and resume behind its all-reduce: the
 * NESVOR_STEP_BIAS_SUM_* flags below.
 * The PSF noise is drawn inside the sampler kernels from (seed, offset) as in nesvor_psf_transform_forward_rng.
 * ---------------------------------------------------------------------- */
#define NESVOR_STEP_MLP_PARTIALS 256
/* nesvor_step_timing: spans of a phase-0 run that are bracketed by HIP events on the stream their launch goes to */
#define NESVOR_STEP_SPAN_PSF_FWD 0
#define NESVOR_STEP_SPAN_HASHGRID_FWD 1
#define NESVOR_STEP_SPAN_MLP_FWD_DENSITY 2
#define NESVOR_STEP_SPAN_MLP_FWD_SIGMA 3
#define NESVOR_STEP_SPAN_LOSS 4
#define NESVOR_STEP_SPAN_MLP_BWD_SIGMA 5
#define NESVOR_STEP_SPAN_MLP_BWD_DENSITY 6
#define NESVOR_STEP_SPAN_HASHGRID_BWD_AGGREGATE 7
#define NESVOR_STEP_SPAN_HASHGRID_BWD_OWNER 8   /* the owner pass; with the fused optimizer: owner pass + the table's AdamW step */
#define NESVOR_STEP_SPAN_PSF_BWD 9
#define NESVOR_STEP_TIMED_SPANS 10
typedef struct {
  nesvor_grid_t grid;
  nesvor_mlp_t density, sigma, bias_net;   /* weights / biases: the model's parameters; bf16_operands: evaluation mode */
  int32_t B, S, n_slices;
  int32_t opt_T, has_lv, has_c, has_lvs, has_b;
  int32_t n_features_z, ks, kb_bias;       /* ks: slice-embedding width fed to sigma_net / b_net (0: none); kb_bias: rows of pe b_net sees */
  int32_t reg_type;                        /* 0 edge, 1 TV, 2 L2 */
  int32_t overlap_owner;                   /* bit 0: owner pass of the hash-grid backward on side_stream; bit 1: a phase-0 run with
                                              `adam` takes the table's AdamW step inside the owner pass (nesvor_hashgrid_backward_adamw;
                                              the table must be the last segment of the flat buffers) */
  float delta, w_T;
  const float *axisangle, *axisangle_init, *psf_sigma, *bounding_box, *logit_coef, *log_var_slice, *slice_embedding, *table;
  float *g_axisangle, *g_logit_coef, *g_log_var_slice, *g_slice_embedding, *g_table, *g_density, *g_sigma, *g_bias_net;
  int32_t n_density_params, n_sigma_params, n_bias_params;  /* columns of a network's partial rows, summed into g_*: W0,b0,W1,b1,..
                                              - or, for a bias-free network (NULL biases, bf16_operands = 4 only), its evaluated weights
                                              W0 | W1 | .. | W_last (out_dim rows): the prefix of its flat gradient; the padding rows
                                              of tinycudann's last layer are never written */
  const float* gw;                         /* 4 upstream gradients d total / d {MSE, logVar, imageReg, biasReg} */
  float *flat_param, *flat_grad, *flat_exp_avg, *flat_exp_avg_sq;
  int64_t flat_numel;
  float *small, *x, *u, *pe, *z, *log_var, *log_bias, *se, *dz, *dlv, *dlb, *dxl, *loss_pix, *pix, *dpe, *dpe_b, *du, *dpix,
      *dxa, *dxa_b, *trans_terms, *g_trans, *lb_mean, *mean_scratch, *partial;
  float* saved_d[NESVOR_MAX_MLP_LAYERS];
  float* saved_s[NESVOR_MAX_MLP_LAYERS];
  float* saved_b[NESVOR_MAX_MLP_LAYERS];
  float* dpre_scratch[NESVOR_MAX_MLP_LAYERS]; /* N_pad16 * 64 floats per hidden layer, shared by the networks' backwards one after the
                                               other; only read for networks nesvor_mlp_backward_fused_ok() refuses (samples per pixel
                                               or pixel features not in multiples of 16 ...): may be NULL when it takes them all */
  void* hg_workspace;
  const float* queue_scale;
  void* side_stream;
} nesvor_step_t;

void* nesvor_step_create(const nesvor_step_t* desc);                 /* NULL on failure */
int nesvor_step_update(void* step, const nesvor_step_t* desc);       /* pointers / sizes changed (e.g. a re-made workspace) */
void nesvor_step_destroy(void* step);
int nesvor_step_run(void* step, const float* xyz, const float* v, const int64_t* slice_idx, uint64_t seed, uint64_t offset,
                    float* losses, int phase, int split_level, const nesvor_adamw_t* adam, void* stream);
/* OR-ed into `phase` (phase 0 with `adam` and overlap_owner bits 0 and 1): return without making `stream` wait for the table's
 * update on side_stream.  The next nesvor_step_run joins it right before its hash-grid forward (its prologue and sampler
 * then overlap the end of this update); anything else that touches the table, its moments or its gradient first calls
 * nesvor_step_join.  Everything but the table (losses, the other parameters) is complete on `stream` as always. */
#define NESVOR_STEP_DEFER_JOIN 8
int nesvor_step_join(void* step, void* stream);
/* The bias field under data parallelism.  biasReg = (mean log_bias)^2 (models.py:322-323) is not a mean of per-sample terms: it needs
 * the mean over ALL ranks' samples, one scalar all-reduce between b_net's forward and the loss kernel.  Two flags, OR-ed into
 * phase 0 or phase 1 (has_b only; never both in one call), run that phase in two calls around the exchange:
 *   NESVOR_STEP_BIAS_SUM_STOP   : prologue, weight norms and images, sampler, hash-grid forward, b_net's input bounds and forward - in
 *                                 FRONT of the density network's, it reads pe and se only - and ONE launch that writes this rank's
 *                                 share of the global mean, sum(log_bias) / (N ranks), into lb_mean; then the call returns.
 *                                 The host sum-all-reduces that one float in place, on any stream ordered behind `stream`.
 *   NESVOR_STEP_BIAS_SUM_RESUME : same arguments.  Density and sigma forwards - they run while the scalar travels - then `stream`
 *                                 waits for the event of nesvor_step_set_bias_mean_event, then the loss kernel and everything
 *                                 behind it, as the un-staged call of that phase (`adam`, NESVOR_STEP_DEFER_JOIN and split_level
 *                                 included).  Weight images, operand bounds, timing spans and the side-stream book-keeping of the
 *                                 first call stay valid for the second, as they do from phase 1 to phase 2.
 * losses[5] (biasReg) is written by the call that completes the step (RESUME at phase 0, phase 2 otherwise): the square of the
 * exchanged mean.  Without the flags a phase-1 / phase-2 pair with has_b uses this rank's own mean (a group of one rank).
 * nesvor_step_set_bias_mean_ranks: the number of ranks W the staged reduction divides by (<= 0 or never set: 1).
 * nesvor_step_set_bias_mean_event: a hipEvent_t recorded behind the all-reduce; consumed by the next RESUME call (the wait is
 * enqueued there, the host never blocks; the event may be destroyed once that call has returned).  NULL, or never set: the
 * caller has ordered `stream` behind the all-reduce itself.
 * These two flags and two entry points were added WITHOUT a change of nesvor_hip_abi_version() (37 then; nothing that existed changed
 * its layout or meaning): the version number does not tell a caller whether they exist - resolve the symbols
 * (dlsym(lib, "nesvor_step_set_bias_mean_event")) to find out; a library without them refuses the flags with hipErrorInvalidValue. */
#define NESVOR_STEP_BIAS_SUM_STOP 16
#define NESVOR_STEP_BIAS_SUM_RESUME 32
int nesvor_step_set_bias_mean_ranks(void* step, int ranks);
int nesvor_step_set_bias_mean_event(void* step, void* event);
/* Per-launch timing of the product step (the roofline leg of bench.py): nesvor_step_timing(handle, 1) makes every following
 * nesvor_step_run bracket the launches listed above with HIP events on the stream each goes to; nesvor_step_timing_read waits
 * for the last run and returns NESVOR_STEP_TIMED_SPANS durations in ms (-1: the span did not occur in that run). */
int nesvor_step_timing(void* handle, int on);
int nesvor_step_timing_read(void* handle, float* ms);

/* ----------------------------------------------------------------------
 * Similarity sums of the stack registration.  Replaces, per optimisation step of `VVR`
 * (nesvor/svort/registration.py:143-247), the K = 1 + 2 x 6 successive evaluations of
 *   warped = F.grid_sample(source, (R_k (points + t_k)) * to_unit, align_corners=True)   (:233-247)
 *   loss(warped, target) reduced over the points                                          (:166-170)
 * by one pass over the points: for every pose k
 *   sums[k] = { sum I, sum I^2, sum I J },  I = source sampled under pose k, J = target;
 *   target_sums = { sum J, sum J^2 } (optional)
 * from which NCC and MSE follow.  source (D,H,W) fp32, points (M,3) physical coordinates, target (M),
 * mats (K,3,4) row-major [R | t] with the translation applied first, to_unit_xyz: HOST pointer to the three factors
 * that map a moved point to grid_sample's normalised coordinates (x, y, z).  sums (K,3) / target_sums (2): fp64,
 * zero-filled by the call.
 * ---------------------------------------------------------------------- */
int nesvor_vvr_similarity(const float* source, int D, int H, int W, const float* points, const float* target,
                          const float* mats, const float* to_unit_xyz, int64_t M, int K, double* sums,
                          double* target_sums, void* stream);

/* ----------------------------------------------------------------------
 * Joint histograms of the stack registration (the statistic of its mutual-information similarity) and the samples behind them.
 * source, points, target, mats, to_unit_xyz (HOST), M, K and the sample I of a (point, pose) are nesvor_vvr_similarity's - one
 * device function serves the three kernels, so I is the same bit for bit; J = target.  EVERY point counts: one that leaves the
 * source has I = 0.
 *   i_lo, i_scale, j_lo, j_scale   the affine maps of I and of J to bin coordinates, one pair each for the call
 *   bins    B, 2 <= B <= 64
 * A value's position on its axis and what a point adds are nesvor_svr_joint_histogram's (below; nesvor_amd/nmi.py): weights
 * 256 - q and q on bins b0 and b0 + 1 of either axis, the four integer products added to cells (bI, bJ), 65536 units per point.
 *   hist[k][bI][bJ]   int64, (K,B,B), row = I bin; fully written (no memset needed); its total is 65536 * M.  Integer adds only: the
 * result does not depend on the order of addition and is the same from run to run.  The point list is cut into segments of 1024
 * to 16384 points (long ones for the 13 poses of a gradient, enough of them to reach about 1024 workgroups for a single pose); a
 * (pose, segment) builds its histogram in LDS in 32-bit cells (16384 points of 65536 units stay below 2^32) and stores it to the
 * workspace, and a second launch adds the segments in 64 bits: no cell overflows at any M.  No float atomic, no global atomic.
 * workspace: device memory of at least nesvor_vvr_joint_histogram_workspace_bytes(M, K, bins) bytes (0 for sizes the call refuses
 * or treats as a no-op).
 * K <= 0 or M <= 0: no-op, returns 0 (hist is not touched).  hipErrorInvalidValue, without a launch: D, H or W below 1, bins
 * outside [2, 64], M above INT_MAX, K times the number of segments above INT_MAX, a workspace that is NULL or too small.
 * nesvor_vvr_sample: out[k][i] = I of point i under pose k, (K,M) fp32, fully written - what nesvor_amd/nmi.py's joint_histogram
 * bins to the very histogram above (the composed path), and the sampling alone for timings.  K <= 0 or M <= 0: no-op;
 * hipErrorInvalidValue: D, H or W below 1, K ceil(M / 256) above INT_MAX.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_vvr_joint_histogram(const float* source, int D, int H, int W, const float* points, const float* target,
                               const float* mats, const float* to_unit_xyz, int64_t M, int K, float i_lo, float i_scale,
                               float j_lo, float j_scale, int bins, int64_t* hist, void* workspace, size_t workspace_bytes,
                               void* stream);
int64_t nesvor_vvr_joint_histogram_workspace_bytes(int64_t M, int K, int bins);
int nesvor_vvr_sample(const float* source, int D, int H, int W, const float* points, const float* mats,
                      const float* to_unit_xyz, int64_t M, int K, float* out, void* stream);

/* ----------------------------------------------------------------------
 * Similarity sums of the slice-to-volume registration: the acquisition operator A (nesvor_slice_acq_forward with
 * interp_psf = 0 and no volume mask) applied to every slice under K poses, reduced at once.  vol (D,H,W) fp32,
 * psf (d_p,h_p,w_p), transforms (n,K,3,4) in A's convention (voxel units), slices (n,h,w) acquired values,
 * slices_mask (n,h,w) bytes or NULL, res_slice the pixel size in voxels.  A pixel is valid under a pose when its mask byte
 * is set (or the mask is NULL) and the PSF weight A finds there is > 0.  Over the valid pixels, I = A's value, J = the
 * acquired value:
 *   sums[i][k] = { count, sum I, sum I^2, sum I J, sum J, sum J^2 }        fp64, (n,K,6), fully written (no memset needed);
 * a (slice, pose) without a valid pixel yields six exact zeros.  The sums are reproducible (no atomics: per-workgroup
 * partials in the workspace, added in workgroup order by a second launch).  workspace: device memory of at least
 * nesvor_svr_similarity_workspace_bytes(n, K, h, w) bytes (0 for sizes the call treats as a no-op).
 * K <= 0 or n == 0: no-op, returns 0.  hipErrorInvalidValue: a size below 1, a PSF of more than 1024 elements
 * (compose the sums from nesvor_slice_acq_forward then), a workspace that is too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_svr_similarity(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                          const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K, int h,
                          int w, float res_slice, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_svr_similarity_workspace_bytes(int n, int K, int h, int w);

/* ----------------------------------------------------------------------
 * Per-slice PSFs: a PSF BANK in A, A^T and the similarity sums (fp32, linear mode; interp_psf, both backwards and fp64 keep
 * one PSF).  A bank is
 *   psf_bank  : P dense PSFs of their own sizes, concatenated into one float array           (device memory)
 *   psf_table : (P,4) int32, row p = { offset of member p in psf_bank in floats, d_p, h_p, w_p }   (HOST memory: the entry
 *               point checks it and hands it to the kernels as an argument; it may be freed when the call returns)
 *   psf_id    : (n) int32, the member of every slice                                           (device memory)
 * Slice k takes member psf_id[k] everywhere: its taps in the order of its dense array with zero taps skipped, its extents
 * in the box bounds of A^T's voxel gather, its weight sum.  The slices are walked in the order k = 0 .. n-1, never grouped
 * by member.  A slice whose id lies outside [0, P) has no taps: it is simulated as empty (no pixel written, no valid pixel
 * in the sums) and contributes nothing to A^T; nothing is indexed by such an id.  With P = 1 and every id 0 the results
 * are those of the one-PSF entry points bit for bit, and so are a member's slices in any bank; a member padded with zero
 * taps gives the same bits as the member itself.
 *
 * Apart from the bank, the arguments, the outputs and the scratch / workspace rules are those of the one-PSF twins:
 *   nesvor_slice_acq_forward_bank          nesvor_slice_acq_forward (interp_psf = 0): writes the pixels of weight > 0 only -
 *                                          the caller zero-fills slices / slices_weight; members of more than 1024 elements
 *                                          are walked from global memory, per slice, in the same launch
 *   nesvor_slice_acq_adjoint_forward_bank  nesvor_slice_acq_adjoint_forward: scratch of 2 n h w floats; vol (and vol_weight, if
 *                                          not NULL) fully written
 *   nesvor_svr_similarity_bank             nesvor_svr_similarity: workspace of nesvor_svr_similarity_workspace_bytes(n, K, h, w);
 *                                          refuses a bank in which ANY member has more than 1024 elements
 * An empty stack (n h w = 0) launches nothing (A^T of it is the zero volume, by clears).
 * hipErrorInvalidValue, before anything is launched or written: P < 1 or P > 32, a NULL bank or table, psf_id NULL with n > 0,
 * a member with a negative offset or a dimension below 1, D H W > INT_MAX, and what the twin refuses.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_slice_acq_forward_bank(const float* transforms, const float* vol, const uint8_t* vol_mask,
                                  const uint8_t* slices_mask, const float* psf_bank, const int32_t* psf_table, int P,
                                  const int32_t* psf_id, float* slices, float* slices_weight, int D, int H, int W, int n,
                                  int h, int w, float res_slice, void* stream);
int nesvor_slice_acq_adjoint_forward_bank(const float* transforms, const float* psf_bank, const int32_t* psf_table, int P,
                                          const int32_t* psf_id, const float* slices, const uint8_t* slices_mask,
                                          const uint8_t* vol_mask, float* vol, float* vol_weight, float* scratch, int D,
                                          int H, int W, int n, int h, int w, float res_slice, int equalize, void* stream);
int nesvor_svr_similarity_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table, int P,
                               const int32_t* psf_id, const float* transforms, const float* slices,
                               const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, double* sums,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------
 * Grouped similarity sums (package registration): the sums of nesvor_svr_similarity for GROUPS of slices that move together.
 * Every slice keeps a base pose, every group takes K corrections, and the call returns the six sums per (group, pose).
 *   base         (n,3,4)   fp32: the pose of every slice, in the storage nesvor_svr_similarity takes (translation first, voxels)
 *   corrections  (G,K,3,4) fp32: same storage
 *   group_offsets (G+1) int32, group_slices (E) int32, E = group_offsets[G]: a CSR grouping in DEVICE memory.  Entry e in
 *                [group_offsets[g], group_offsets[g+1]) says that slice group_slices[e] belongs to group g.  Offsets start at 0
 *                and do not decrease; a group may be empty, a slice may be listed nowhere (it takes no part) or more than once.
 *                The CALLER guarantees this and 0 <= group_slices[e] < n (the library cannot read device memory on the host;
 *                torch.ops.nesvor.svr_similarity_groups checks both on the host before it uploads them).  An index outside
 *                [0, n) is never used to index anything: its entry counts no pixel.
 * The pose of slice i of group g under pose k is  corrections[g][k] o base[i]  in the sense of RigidTransform.compose:
 *   R'[r][c] = Rc[r][0] R[0][c] + Rc[r][1] R[1][c] + Rc[r][2] R[2][c]
 *   t'[r]    = t[r] + (R[0][r] uc[0] + R[1][r] uc[1] + R[2][r] uc[2])
 * in double from the fp32 inputs, every sum added left to right without contraction, rounded once to fp32; once per
 * workgroup.  From that matrix on a pixel's value and valid set are nesvor_svr_similarity's bit for bit, and so are an
 * entry's sums (workgroup rows added from 0).  sums (G,K,6) fp64: a group's sum adds its entries' sums one after the other
 * from 0 in CSR order - "nesvor_svr_similarity at the composed matrices, added per group in CSR order", bit for bit; an empty
 * group gives six zeros.  No atomics, no memset.  The grid runs over the E entries: a subset of the slices costs what it holds.
 * workspace: nesvor_svr_similarity_groups_workspace_bytes(E, K, h, w) bytes.
 * K <= 0 or E == 0: returns 0 without a launch and WITHOUT writing sums.  hipErrorInvalidValue: what nesvor_svr_similarity
 * (the bank twin: nesvor_svr_similarity_bank) refuses, G < 1, E < 0, NULL group_offsets, NULL group_slices with E > 0.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_svr_similarity_groups(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                                 const float* base, const float* corrections, const int32_t* group_offsets,
                                 const int32_t* group_slices, int G, int E, const float* slices, const uint8_t* slices_mask,
                                 int n, int K, int h, int w, float res_slice, double* sums, void* workspace,
                                 size_t workspace_bytes, void* stream);
int nesvor_svr_similarity_groups_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table,
                                      int P, const int32_t* psf_id, const float* base, const float* corrections,
                                      const int32_t* group_offsets, const int32_t* group_slices, int G, int E,
                                      const float* slices, const uint8_t* slices_mask, int n, int K, int h, int w,
                                      float res_slice, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_svr_similarity_groups_workspace_bytes(int E, int K, int h, int w);

/* ----------------------------------------------------------------------
 * Joint histograms of the slice-to-volume registration (the statistic of its mutual-information similarity): what
 * nesvor_svr_similarity sums into six moments, binned.  vol, psf, transforms (n,K,3,4), slices, slices_mask, res_slice and the
 * valid set (mask byte set or mask NULL, PSF weight > 0) are nesvor_svr_similarity's; I = A's value, J = the acquired value.
 *   i_lo, i_scale        the affine map of I to bin coordinates, one for the call
 *   j_map   (n,2) fp32   { lo, scale } of J per slice (device memory)
 *   bins    B, 2 <= B <= 64
 * Position of a value v on an axis, in fp32 with every operation rounded on its own:
 *   u = clamp((v - lo) * scale, 0, B-1),  b0 = min((int)u, B-2),  f = u - b0,  q = (int)(f * 256 + 0.5)   in [0, 256]
 * v gives weight 256 - q to bin b0 and q to bin b0 + 1.  A valid pixel adds the four integer products of its I weights and its
 * J weights to cells (bI, bJ): 65536 units per pixel.
 *   hist[i][k][bI][bJ]   int64, (n,K,B,B), row = I bin; fully written (no memset needed); its total is 65536 * count, a
 * (slice, pose) without a valid pixel yields zeros.  Integer adds only: the result does not depend on the order of addition and
 * is the same from run to run.  A slice's pixels are cut into segments of 1024 to 16384 pixels (whole slices when n K reaches 1024
 * workgroups, shorter segments for smaller calls); a segment's histogram is built in LDS in 32-bit cells (16384 pixels of 65536
 * units stay below 2^32), stored to the workspace, and a second launch adds the segments in 64 bits: no cell overflows at any
 * slice size.  workspace: device memory of at least
 * nesvor_svr_joint_histogram_workspace_bytes(n, K, h, w, bins) bytes (0 for sizes the call refuses or treats as a no-op).
 * K <= 0 or n == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: what nesvor_svr_similarity refuses (the bank
 * twin: nesvor_svr_similarity_bank), bins outside [2, 64], NULL j_map, a workspace that is NULL or too small.
 * nesvor_svr_joint_histogram_bank: the PSF-bank twin ((psf_bank, psf_table (host), P, psf_id) in the place of (psf, d_p, h_p,
 * w_p)); the workspace size does not differ.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_svr_joint_histogram(const float* vol, int D, int H, int W, const float* psf, int d_p, int h_p, int w_p,
                               const float* transforms, const float* slices, const uint8_t* slices_mask, int n, int K, int h,
                               int w, float res_slice, float i_lo, float i_scale, const float* j_map, int bins, int64_t* hist,
                               void* workspace, size_t workspace_bytes, void* stream);
int nesvor_svr_joint_histogram_bank(const float* vol, int D, int H, int W, const float* psf_bank, const int32_t* psf_table,
                                    int P, const int32_t* psf_id, const float* transforms, const float* slices,
                                    const uint8_t* slices_mask, int n, int K, int h, int w, float res_slice, float i_lo,
                                    float i_scale, const float* j_map, int bins, int64_t* hist, void* workspace,
                                    size_t workspace_bytes, void* stream);
int64_t nesvor_svr_joint_histogram_workspace_bytes(int n, int K, int h, int w, int bins);

/* ----------------------------------------------------------------------
 * One descent step of the classical super-resolution reconstruction with the edge-preserving prior, in one launch
 * (the loop body of the reference's SRR, svort/srr.py:117-131, whose prior gradient dR is :139-160):
 *   out[a] = x[a] - alpha * (grad[a] + beta * dR(x)[a])
 * x, grad, out (D,H,W) fp32.  For an interior voxel dR is the sum over its 26 neighbours o of  t / sqrt(1 + d t),
 * d = x[a] - x[a+o], t = d / (|o|^2 delta^2); dR is 0 on every border voxel (everywhere when min(D,H,W) < 3), where the
 * result is x - alpha * grad exactly.  beta is the effective multiplier (the reference's beta * delta^2).  clamp != 0:
 * negative results become 0, NaN stays NaN.  The 26 terms are added in a fixed order without atomics: bit-reproducible.
 * out == grad is allowed (saves a buffer).  hipErrorInvalidValue, without a launch: a null pointer, a dimension below 1,
 * D H W > INT_MAX, out overlapping x (the stencil reads neighbours), out overlapping grad partially.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbol to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_srr_step(const float* x, const float* grad, float* out, int D, int H, int W, float alpha, float beta,
                    float delta, int clamp, void* stream);

/* ----------------------------------------------------------------------
 * E-step of the robust statistics of the classical reconstruction (nesvor_amd/robust.py; the EM scheme of
 * Kuklisova-Murgasova et al. 2012): pixel posteriors and the per-slice sums of one EM round in one pass.
 * sim (n,h,w) fp32 the simulated slices A x, y (n,h,w) fp32 the acquired ones, mask (n,h,w) bytes or NULL, scale (n) fp32,
 * model: three DEVICE floats {sigma2, c, m} (read by the kernel: the caller's loop needs no host synchronisation).
 * For a valid pixel (mask NULL or its byte set) of slice k
 *   e = scale[k] * y - sim,   g = exp(-e^2 / (2 sigma2)) / sqrt(2 pi sigma2),   p = c g / (c g + (1 - c) m);
 * p = 0 on every other pixel.  p (n,h,w) fp32 and stats (n,7) fp64 are fully written (no memset needed):
 *   stats[k] = { n_k, sum p, sum p e^2, sum (1 - p)^2, sum p y sim, sum p y^2, sum e^2 }   over the valid pixels of slice k;
 * a slice without a valid pixel yields seven exact zeros, n_k is exact.  The sums are reproducible (no atomics: per-workgroup
 * partials in the workspace, added in workgroup order by a second launch).  workspace: device memory of at least
 * nesvor_robust_estep_workspace_bytes(n, h, w) bytes (0 for sizes the call treats as a no-op or refuses).
 * n == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: n < 0, h or w below 1, h w > INT_MAX - 256, more than
 * INT_MAX workgroups (n * ceil(h w / 256)), a null pointer other than mask, a workspace that is missing or too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_robust_estep(const float* sim, const float* y, const uint8_t* mask, const float* scale, const float* model, int n,
                        int h, int w, float* p, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_robust_estep_workspace_bytes(int n, int h, int w);

/* ----------------------------------------------------------------------
 * Masked moments of slice pairs, the sums the stack quality scores are functions of (nesvor_amd/assess.py): NCC of
 * adjacent slices, the Gram matrix of a stack.  slices (n,h,w) fp32, mask (n,h,w) bytes or NULL, pairs (P,2) DEVICE int32.
 * For pair p = (a, b) over the pixels valid in both slices (both mask bytes set; every pixel when mask is NULL)
 *   moments[p] = { count, sum a, sum b, sum a^2, sum b^2, sum a b }        fp64, (P,6), fully written (no memset needed);
 * a pair without a common valid pixel yields six exact zeros, the count is exact.  Products are fp32, sums fp32 inside one
 * wave (64 terms) and fp64 beyond; reproducible (no atomics: per-workgroup partials in the workspace, added in workgroup
 * order by a second launch).  Self-pairs and repeated pairs are legal; (b, a) yields the bits of (a, b) with columns
 * 1 <-> 2 and 3 <-> 4 swapped.  The pair indices are NOT checked on the device: the caller range-checks them (0 <= index < n)
 * on the host before the upload.  workspace: device memory of at least nesvor_pair_moments_workspace_bytes(P, h, w) bytes
 * (0 for sizes the call treats as a no-op or refuses).
 * P == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: P < 0, n, h or w below 1, h w > INT_MAX - 256, more than
 * INT_MAX workgroups (P * ceil(h w / 256)), a null pointer other than mask, a workspace that is missing or too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_pair_moments(const float* slices, const uint8_t* mask, int n, int h, int w, const int32_t* pairs, int P,
                        double* moments, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_pair_moments_workspace_bytes(int P, int h, int w);

/* ----------------------------------------------------------------------
 * Bias field correction (nesvor_amd/bias.py; N4-style: histogram sharpening and a multilevel cubic B-spline fit of the log
 * field): the three per-iteration passes over a stack taken as a (D,H,W) array in index space.  Common to all three:
 * v (D,H,W) fp32 the log intensities, f (D,H,W) fp32 the log field, mask (D,H,W) bytes or NULL (any set byte = valid voxel,
 * NULL = all valid), u = v - f in double.  range: two DEVICE floats {lo, hi} (read by the kernels: the caller's loop needs no
 * host synchronisation); slope = (hi - lo) / (n_bins - 1) and the bin coordinate c = (u - lo) / slope clamped to
 * [0, n_bins - 1] (a NaN counts as 0), both in double.  The B-spline lattice has S spans and C = S + 3 control points per
 * axis; per axis a table pair of the voxel indices 0 .. n - 1: s* (n) int32 the first control index (clamped to [0, S - 1] on
 * the device) and t* (n,4) fp32 the four uniform cubic basis values on control indices s .. s + 3.  Results are fully
 * written (no memset needed) and bit-identical from run to run: no floating-point atomics; fp32 sums only inside one wave
 * (64 terms), fp64 beyond; partials in the workspace, added in a fixed order by small follow-up launches.  workspace: device
 * memory of at least the matching *_workspace_bytes(...) bytes (0 for sizes the call refuses).
 * hipErrorInvalidValue, without a launch: a null pointer other than mask, a dimension below 1, D H W > INT_MAX - 256,
 * S < 1 or C > 16, n_bins < 2 or n_bins > 1024, a workspace that is missing or too small.
 *
 * nesvor_n4_histogram: hist (n_bins) fp64, the fractionally binned histogram of u over the valid voxels: with
 *   i = min(floor c, n_bins - 2) a voxel adds 1 - (c - i) to bin i and c - i to bin i + 1.  Integer LDS atomics on fixed-point
 *   weights with the quantum 2^-32 (a voxel adds round((c - i) 2^32) and 2^32 minus that: the total is the exact count; a
 *   bin is within 2^-33 per touching voxel of the fp64 sum), per-workgroup 64-bit bins added by the second launch.
 * nesvor_n4_fit: lut (n_bins) fp64 the sharpened histogram's conditional expectation E; the residual of a valid voxel is
 *   r = u - (E[j] (1 - t) + E[j+1] t), j = min(floor c, n_bins - 2), t = c - j.  With w_k the product of a voxel's three axis
 *   weights on control point k:  weight[k] = sum_p w_kp^2,  lattice[k] = sum_p w_kp^3 r_p / (sum_c w_cp^2) / weight[k]
 *   (0 where weight[k] is 0), both (C,C,C) fp64, over the valid voxels p.  One pass contracts x per (z,y) row, two small
 *   launches contract y, then z, in ascending index order.
 * nesvor_n4_update: f += sum_k lattice[k] w_k IN PLACE on every voxel (the sum in double, rounded once); stats: five fp64
 *   {count, sum g, sum g^2, min u_new, max u_new} over the valid voxels, g = expm1(the voxel's increment), u_new = v - f_new
 *   (+inf / -inf without a valid voxel): the stop test and the next iteration's range.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_n4_histogram(const float* v, const float* f, const uint8_t* mask, int D, int H, int W, const float* range,
                        int n_bins, double* hist, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_n4_histogram_workspace_bytes(int D, int H, int W, int n_bins);
int nesvor_n4_fit(const float* v, const float* f, const uint8_t* mask, const float* range, const double* lut, int n_bins,
                  const float* tz, const float* ty, const float* tx, const int32_t* sz, const int32_t* sy, const int32_t* sx,
                  int D, int H, int W, int S, double* lattice, double* weight, void* workspace, size_t workspace_bytes,
                  void* stream);
int64_t nesvor_n4_fit_workspace_bytes(int D, int H, int W, int S);
int nesvor_n4_update(const double* lattice, const float* tz, const float* ty, const float* tx, const int32_t* sz,
                     const int32_t* sy, const int32_t* sx, int S, float* f, const float* v, const uint8_t* mask, int D, int H,
                     int W, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_n4_update_workspace_bytes(int D, int H, int W);

/* ----------------------------------------------------------------------
 * Structural exclusion of the classical reconstruction (nesvor_amd/structural.py): the local SSIM map of the acquired slices
 * against the simulated ones and the per-slice sums of the slice similarity in one pass.
 * sim (n,h,w) fp32 the simulated slices A x, y (n,h,w) fp32 the acquired ones, mask (n,h,w) bytes or NULL, scale (n) DEVICE
 * fp32.  With I = scale[k] y and J = sim on the valid pixels (mask NULL or its byte set) and 0 elsewhere, v the validity as
 * 0 / 1 and S the separable 11-tap Gaussian window (sigma 1.5, taps normalised to sum 1, zero padding, along x first, taps
 * added in ascending order from 0):
 *   Wt = S(v),  muI = S(I) / Wt,  muJ = S(J) / Wt,  sI = S(I I) / Wt - muI^2,  sJ = S(J J) / Wt - muJ^2,  sIJ = S(I J) / Wt - muI muJ,
 *   ssim = (2 muI muJ + c1) (2 sIJ + c2) / ((muI^2 + muJ^2 + c1) (sI + sJ + c2))       at valid pixels, 0 on every other pixel,
 * all in fp32 without contraction.  ssim (n,h,w) fp32 and stats (n,8) fp64 are fully written (no memset needed):
 *   stats[k] = { n_k, sum ssim, #(ssim < threshold), sum I, sum J, sum I^2, sum J^2, sum I J }   over the valid pixels of slice k;
 * a slice without a valid pixel yields eight exact zeros, both counts are exact.  Products are fp32, the sums double from the
 * first add.  The sums are reproducible (no atomics:
 * per-workgroup partials in the workspace, added in workgroup order by a second launch).  workspace: device memory of at
 * least nesvor_structural_ssim_workspace_bytes(n, h, w) bytes (0 for sizes the call treats as a no-op or refuses).
 * n == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: n < 0, h or w below 1, h w > INT_MAX - 256, more than
 * INT_MAX workgroups (n * ceil(h / 16) * ceil(w / 16)), a null pointer other than mask, a workspace that is missing or too
 * small, a negative or non-finite c1, c2 or threshold.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_structural_ssim(const float* sim, const float* y, const uint8_t* mask, const float* scale, int n, int h, int w,
                           float c1, float c2, float threshold, float* ssim, double* stats, void* workspace,
                           size_t workspace_bytes, void* stream);
int64_t nesvor_structural_ssim_workspace_bytes(int n, int h, int w);

/* ----------------------------------------------------------------------
 * Stack masking (nesvor_amd/masking.py): which voxels of a stack count.  slices (n,h,w) fp32, mask (n,h,w) bytes or NULL
 * (any set byte = valid, NULL = all valid), transforms (n,3,4) fp32 the slices' poses [R | t] with x' = R (x + t).  Pixel
 * (r, c) of slice s lies at p = R_s (x + t_s), x = ((c - (w - 1) / 2) rx, (r - (h - 1) / 2) ry, 0); positions and tests are
 * double.  Results are fully written (no memset needed) and bit-identical from run to run: no global atomics, per-workgroup
 * partials in the workspace combined in workgroup order by small follow-up launches, integer LDS atomics in the histogram.
 * workspace: device memory of at least the matching *_workspace_bytes(...) bytes (0 for sizes the call refuses, and for
 * nesvor_otsu_threshold, which needs none and ignores the argument).
 * hipErrorInvalidValue, without a launch: a null pointer other than the optional ones named below, a dimension below 1,
 * h w > INT_MAX - 256, more than INT_MAX workgroups (n * ceil(h w / 256)), n_bins < 2 or n_bins > 1024, a workspace that is
 * missing or too small; nesvor_stack_mask also: rx or ry not positive and finite, a volume without volume_geometry or with
 * a dimension below 1 or more than INT_MAX voxels, n_others or n_slabs below 0, n_others > 0 with a null slab table;
 * nesvor_otsu_histogram also: n h w > INT_MAX - 256.
 *
 * nesvor_stack_mask: out_mask (n,h,w) bytes 0 / 1 and stats (n,3) fp64 {count, min, max} of the kept intensities per slice
 *   (+inf / -inf without one; a NaN intensity never enters min or max; the count is exact).  A valid voxel is kept if it
 *   passes every rule that is given, in this order:
 *   threshold (one DEVICE float or NULL): intensity > threshold[0] (false for a NaN);
 *   volume (vd,vh,vw) bytes or NULL with volume_geometry, 15 DEVICE doubles: the world-to-lattice matrix (3,4) [M | t] and
 *     the voxel sizes {x, y, z}: with u = (M p + t) / size + (shape_xyz - 1) / 2 the trilinear interpolation of the 0 / 1
 *     array (any set byte = 1, 0 off the lattice) at u is >= 0.5;
 *   slabs (n_slabs,3,4) DEVICE doubles, the world-to-slice matrices [M | t] (q = M p + t) of the slices of n_others other
 *     stacks, stack k owning rows slab_offsets[k] .. slab_offsets[k + 1] - 1 (DEVICE int32, n_others + 1, clamped to the
 *     table on the device) with the half-extents slab_extents[k] = {x, y, z} (DEVICE doubles): for every k some row has
 *     |q_x| <= x, |q_y| <= y and |q_z| <= z.  n_others == 0: no such rule.  The table goes through LDS 64 rows at a time.
 * nesvor_otsu_histogram: hist (n_bins) int64, the counts of the valid voxels' intensities v over range = two DEVICE
 *   doubles {lo, hi}: bin min(floor((v - lo) / ((hi - lo) / n_bins)), n_bins - 1), the coordinate in double; a voxel whose
 *   coordinate is not >= 0 (a NaN intensity, a flat or empty range) is not counted.
 * nesvor_otsu_threshold: threshold, one DEVICE float: with the bin centres m_i = lo + (i + 0.5) (hi - lo) / n_bins and, for
 *   the split after bin i (i = 0 .. n_bins - 2), var_i = w0 w1 (mu0 - mu1)^2 from the class weights and the class means of the
 *   centres (0 where a class is empty), in double, the running sums added in ascending bin order: (float) m_i of the first
 *   maximum; -inf for fewer than two counted voxels or a range that is not lo < hi.  One workgroup.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_stack_mask(const float* slices, const uint8_t* mask, const float* transforms, int n, int h, int w, double rx,
                      double ry, const float* threshold, const uint8_t* volume, int vd, int vh, int vw,
                      const double* volume_geometry, const double* slabs, const double* slab_extents,
                      const int32_t* slab_offsets, int n_others, int n_slabs, uint8_t* out_mask, double* stats,
                      void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_stack_mask_workspace_bytes(int n, int h, int w);
int nesvor_otsu_histogram(const float* slices, const uint8_t* mask, int n, int h, int w, const double* range, int n_bins,
                          int64_t* hist, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_otsu_histogram_workspace_bytes(int n, int h, int w, int n_bins);
int nesvor_otsu_threshold(const int64_t* hist, const double* range, int n_bins, float* threshold, void* workspace,
                          size_t workspace_bytes, void* stream);
int64_t nesvor_otsu_threshold_workspace_bytes(int n_bins);

/* ----------------------------------------------------------------------
 * Slice bias fields of the classical reconstruction (nesvor_amd/slice_bias.py): one round of the smooth multiplicative field
 * of every slice, estimated from the log-ratio of the slice to its simulation.
 * sim (n,h,w) fp32 the simulated slices A x, y (n,h,w) fp32 the acquired ones, mask (n,h,w) bytes or NULL, scale (n) DEVICE
 * fp32, weight (n,h,w) fp32 the pixel weights or NULL (ones), b (n,h,w) fp32 the current log-field.  With lo = min_intensity,
 *   e = valid & (y > lo) & (sim > lo)   (valid: mask NULL or its byte set),
 *   I = (scale[k] y) exp(-b),  r = clamp(log(I / sim), -log 2, log 2),  u = weight   on the eligible pixels, r = u = 0 elsewhere,
 * and S the separable Gaussian window of `radius` R (2 R + 1 taps exp(-(t - R)^2 / (2 sigma_px^2)) normalised to sum 1 in
 * double and rounded to fp32, zero padding, along x first, taps added in ascending order from 0):
 *   num = S(u r),  den = S(u),  b_new = b + (den > 1e-3 ? num / den : 0)                                 on every pixel,
 * all in fp32 without contraction.  b_new (n,h,w) fp32 and stats (n,5) fp64 are fully written (no memset needed):
 *   stats[k] = { #e, sum u, sum u b_new, sum u r, sum (u r) r }   over the eligible pixels of slice k;
 * a slice without one yields five exact zeros, the count is exact.  Products are fp32, the sums double from the first add.
 * The sums are reproducible (no atomics: per-workgroup partials in the workspace, added in workgroup order by a third
 * launch).  Centring a field and the rule for slices of little weight are the caller's (slice_bias.py).  workspace: device
 * memory of at least nesvor_slice_bias_update_workspace_bytes(n, h, w) bytes (the partial sums and the two row-filtered
 * intermediates; 0 for sizes the call treats as a no-op or refuses).
 * n == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: n < 0, h or w below 1, h w > INT_MAX - 256, more than
 * INT_MAX workgroups in either pass, a null pointer other than mask and weight, b_new == b (the row pass reads the
 * neighbours' b), radius < 1 or radius > 48, a sigma_px that is not positive and finite, a workspace that is missing or too
 * small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_slice_bias_update(const float* sim, const float* y, const uint8_t* mask, const float* scale, const float* weight,
                             const float* b, int n, int h, int w, double sigma_px, int radius, float min_intensity, float* b_new,
                             double* stats, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_slice_bias_update_workspace_bytes(int n, int h, int w);

/* ----------------------------------------------------------------------
 * Stack denoising (nesvor_amd/denoise.py): 2-D non-local means of every slice of a stack, slice by slice.
 * y (n,h,w) fp32 the slices, mask (n,h,w) bytes or NULL (all valid), sigma (n) DEVICE fp32 the noise standard deviation of
 * every slice, P = patch_radius in 1 .. 3, S = search_radius in 1 .. 10, beta = strength.  With m the validity as 0 / 1 (0
 * outside the image), y0 = y on valid pixels and 0 elsewhere, and for a valid pixel p of slice k with sigma_k positive and finite:
 *   candidates   q = p + t, t in [-S,S]^2 \ {0} with m(q) = 1, taken in ascending (t_y, t_x);
 *   c_o = m(p+o) m(q+o),  e_o = c_o (y0(p+o) - y0(q+o))^2,  o in [-P,P]^2;  num = sum_o e_o and den = sum_o c_o, each added
 *                along x first and then along y, in ascending order from the first term;
 *   d2 = num / max(den, 1),   w(p,q) = exp(-(max(d2 - 2 sigma_k^2, 0) / (beta sigma_k)^2));
 *   w_c = the largest w(p,q), or 1 without a candidate;  W = w_c + sum_q w(p,q),  V = w_c y(p) + sum_q w(p,q) y(q);
 *   out(p) = V / W, or y(p) where W is 0 (every weight underflowed),
 * all in fp32 without contraction, expf the library's, the sums over q from 0 in candidate order.  An invalid pixel and every
 * pixel of a slice whose sigma_k is not positive and finite keep y bit for bit.  out (n,h,w) fp32 and stats (n,2) fp64 are
 * fully written (no memset needed):  stats[k] = { number of valid pixels, sum over them of (out - y)^2 }, the count exact, the
 * squares fp32, their sum double from the first add and reproducible (no atomics: per-workgroup partials in the workspace,
 * added in workgroup order by a second launch).  One workgroup per 16 x 16 tile of a slice; y is read once per tile (with its
 * S + P halo) into LDS and nothing else is read.  workspace: device memory of at least
 * nesvor_nlm_denoise_workspace_bytes(n, h, w) bytes (0 for sizes the call treats as a no-op or refuses).
 * n == 0: no-op, returns 0.  hipErrorInvalidValue, without a launch: n < 0, h or w below 1, h w > INT_MAX - 256, more than
 * INT_MAX workgroups, a null pointer other than mask, out == y (a tile reads its neighbours' y), patch_radius outside 1 .. 3,
 * search_radius outside 1 .. 10, a strength that is not positive and finite, a workspace that is missing or too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_nlm_denoise(const float* y, const uint8_t* mask, const float* sigma, int n, int h, int w, int patch_radius,
                       int search_radius, float strength, float* out, double* stats, void* workspace, size_t workspace_bytes,
                       void* stream);
int64_t nesvor_nlm_denoise_workspace_bytes(int n, int h, int w);

/* ----------------------------------------------------------------------
 * Volume comparison (nesvor_amd/evaluate.py, the `evaluate` command): a volume X on the lattice of a reference volume R, and
 * the 3-D SSIM map of the two with the sums of the error measures.
 *
 * nesvor_volume_resample.  reference (d,h,w) fp32 = I0 with reference_mask (d,h,w) bytes or NULL (all set), volume
 * (vd,vh,vw) fp32 = X0 with volume_mask (vd,vh,vw) bytes or NULL; any set byte counts.  index_map: 12 HOST doubles, M (3,4)
 * row-major, taking an R voxel index (x, y, z) to the continuous X voxel index in double, in the written order:
 *   u_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3],       a = 0, 1, 2 = the x, y, z axis of X (sizes vw, vh, vd).
 * With eps = 2^-20 the voxel is inside where -eps <= u_a <= size_a - 1 + eps on the three axes; u is then clamped to
 * [0, size - 1]; i0 = floor(u), f = (float)(u - floor(u)), i1 = min(i0 + 1, size - 1).  lerp(a, b, f) = a + f (b - a) in fp32
 * without contraction, along x, then y, then z, interpolates J0 from X0 and mX from the volume mask as 0 / 1 (1 if NULL):
 *   v = reference mask and inside and mX >= 0.5,      resampled = J0 on v and 0 elsewhere,      valid = v as 0 / 1.
 * resampled (d,h,w) fp32, valid (d,h,w) bytes and stats (8) fp64 are fully written (no memset needed):
 *   stats = { n = #v, n_ref = #reference mask, sum I, sum J, sum I^2, sum J^2, sum I J, max I }     over v, I = I0, J = J0;
 * the counts and the maximum (-inf without a valid voxel) are exact, products are fp32, the sums double from the first add
 * and reproducible (no atomics: per-workgroup partials in the workspace, combined in a fixed order by a second launch).
 *
 * nesvor_volume_ssim.  reference, resampled, valid as above, params a DEVICE float[4] = {a, b, c1, c2}.  With I = I0 and
 * J' = a J0 + b (a multiply, then an add) on v and 0 elsewhere, and S the separable 11-tap Gaussian window of
 * nesvor_structural_ssim with zero padding along x, then y, then z, taps added in ascending order from 0:
 *   Wt = S(v),  muI = S(I) / Wt,  muJ = S(J') / Wt,  sI = S(I I) / Wt - muI^2,  sJ = S(J' J') / Wt - muJ^2,  sIJ = S(I J') / Wt - muI muJ,
 *   ssim = (2 muI muJ + c1) (2 sIJ + c2) / ((muI^2 + muJ^2 + c1) (sI + sJ + c2))          on v, 0 on every other voxel,
 * all in fp32 without contraction.  ssim (d,h,w) fp32 and stats (4) fp64 are fully written:
 *   stats = { n, sum ssim, sum e^2, sum |e| }     over v, e = I - J';
 * n is exact, the sums double from the first add and reproducible.  A workgroup owns a 16 x 16 in-plane tile and 32
 * consecutive planes (EVALUATE_Z_CHUNK of nesvor_amd/ops.py).  ssim must not overlap an input.
 *
 * workspace: device memory of at least nesvor_volume_*_workspace_bytes(d, h, w) bytes (0 for sizes the call refuses):
 * 64 bytes per 256 voxels for the resampling, 32 bytes per (16 x 16 tile, 32 planes) for the SSIM.
 * hipErrorInvalidValue, without a launch: a null pointer other than the two masks, a dimension (of either volume) below 1,
 * more than INT_MAX - 256 voxels (in either volume), more than INT_MAX workgroups, a non-finite entry of index_map, a
 * workspace that is missing or too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_volume_resample(const float* reference, const uint8_t* reference_mask, int d, int h, int w, const float* volume,
                           const uint8_t* volume_mask, int vd, int vh, int vw, const double* index_map, float* resampled,
                           uint8_t* valid, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_volume_resample_workspace_bytes(int d, int h, int w);
int nesvor_volume_ssim(const float* reference, const float* resampled, const uint8_t* valid, const float* params, int d, int h,
                       int w, float* ssim, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_volume_ssim_workspace_bytes(int d, int h, int w);

/* ----------------------------------------------------------------------
 * Moment sums of K candidate poses in one pass over the reference (nesvor_amd/align.py, `evaluate --align`).
 *
 * nesvor_volume_pose_moments.  The volumes and masks are nesvor_volume_resample's.  index_maps: K x 12 HOST doubles, K index
 * maps (3,4) row-major, 1 <= K <= 16 (they travel as kernel arguments).  For every map the per-voxel arithmetic and the
 * validity rule v are nesvor_volume_resample's, operation for operation (one device routine serves both), and
 *   sums[k] = { n = #v, sum I, sum J, sum I^2, sum J^2, sum I J }     over v, I = I0, J = J0
 * are entries 0, 2, 3, 4, 5, 6 of that call's stats.  sums (K,6) fp64 is fully written.  n is exact, products are fp32, the
 * sums double from the first add.  No atomics: a workgroup owns 1024 consecutive voxels (EVALUATE_POSE_CHUNK of
 * nesvor_amd/ops.py), thread t of it the voxels t, t + 256, t + 512, t + 768, whatever K is; per-workgroup partials go to the
 * workspace and a second launch adds them in a fixed order.  Which thread owns a voxel and the order of every add depend on
 * (d, h, w) alone: the six sums of a pose are bit-identical whatever else is in the call, and from run to run.
 * The reference value and mask byte of a voxel are read once for the K poses; a voxel off the reference mask or outside the
 * volume under a pose gathers nothing for it; 8 gathers per pose without a volume mask, 16 with one.
 *
 * workspace: at least nesvor_volume_pose_moments_workspace_bytes(d, h, w, K) = 48 K ceil(d h w / 1024) bytes of device memory
 * (0 for sizes and K the call refuses, and for K = 0).
 * K = 0 returns 0 without a launch.  hipErrorInvalidValue, without a launch: K < 0 or K > 16, a null pointer other than the
 * two masks, a dimension (of either volume) below 1, more than INT_MAX - 256 voxels (in either volume), a non-finite map
 * entry, a workspace that is missing or too small.
 * (Added without a change of nesvor_hip_abi_version(): nothing that existed changed; resolve the symbols to find out.)
 * ---------------------------------------------------------------------- */
int nesvor_volume_pose_moments(const float* reference, const uint8_t* reference_mask, int d, int h, int w, const float* volume,
                               const uint8_t* volume_mask, int vd, int vh, int vw, const double* index_maps, int K, double* sums,
                               void* workspace, size_t workspace_bytes, void* stream);
int64_t nesvor_volume_pose_moments_workspace_bytes(int d, int h, int w, int K);

#ifdef __cplusplus
}
#endif
#endif /* NESVOR_HIP_H */
