"""Compare the kernels of two gfx950 assembly files (hipcc --cuda-device-only -S of the same unit before and after a change):

    python tools/asm_diff.py old.s new.s [old_name=new_name ...]        exit status 1 if any kernel is different

A kernel's instruction stream (check_inflight_loads.parse: instructions and block labels, comments stripped) is compared after
the compiler's local label numbers - .LBB<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>, which move with the function's index
in the file - are mapped to one token; its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor block (registers, LDS, scratch)
is compared line for line.  Kernels are matched by mangled name; a renamed kernel (a template parameter dropped) is given as
old_name=new_name.  Lists the kernels gone, new, identical and different.
"""
import re
import sys

import check_inflight_loads as chk

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")  # (the block number behind .LBB<n>_ stays: a branch to another block is a change)


def descriptors(path):
    out, name = {}, None
    for line in open(path):
        t = line.split(";")[0].strip()
        if t.startswith(".amdhsa_kernel "):
            name, out[t.split()[1]] = t.split()[1], []
        elif t.startswith(".end_amdhsa_kernel"):
            name = None
        elif name is not None and t:
            out[name].append(t)
    return out


def kernels(path):
    """name -> (normalised body, descriptor lines)"""
    desc = descriptors(path)
    return {n: ([LOCAL.sub(r".L\1", t) for t in body], desc.get(n)) for n, body in chk.parse(path).items() if n in desc}


def compare(old_path, new_path, renames=()):
    """(gone, new, identical, different): lists of names (the old name of a renamed kernel)"""
    old, new = kernels(old_path), kernels(new_path)
    to_new = dict(renames)
    pairs = {o: to_new.get(o, o) for o in old}
    gone = sorted(o for o, n in pairs.items() if n not in new)
    fresh = sorted(set(new) - set(pairs.values()))
    same = sorted(o for o, n in pairs.items() if n in new and old[o] == new[n])
    diff = sorted(o for o, n in pairs.items() if n in new and old[o] != new[n])
    return gone, fresh, same, diff


if __name__ == "__main__":
    gone, fresh, same, diff = compare(sys.argv[1], sys.argv[2], [a.split("=", 1) for a in sys.argv[3:]])
    for title, names in (("gone", gone), ("new", fresh), ("different", diff)):
        for n in names:
            print(f"{title}: {n}")
    print(f"{len(gone)} gone, {len(fresh)} new, {len(same)} identical, {len(diff)} different")
    sys.exit(1 if diff else 0)
