"""Static VALU and spill-lane counts of kernels in two `hipcc -S --offload-device-only` listings.

  python tools/valu_count.py OLD.s NEW.s [substring of the demangled kernel name ...]

Per kernel (metadata order of OLD.s; the same mangled name in NEW.s): VGPRs, SGPR spills and scratch from the
metadata, then the listing's instructions, its VALU instructions (mnemonic v_*) and, among those, the lane
reads / writes that move spilled scalars (v_readlane_b32 / v_writelane_b32).  With name substrings, only
the kernels whose demangled name contains every one of them.
"""
import re
import sys

from isa_compare import demangle, parse, res


def counts(body):
    valu = [t for t in body if t.startswith("v_")]
    lanes = [t for t in valu if t.startswith(("v_readlane_b32", "v_writelane_b32"))]
    f64 = [t for t in valu if re.match(r"v_\w+_f64", t)]
    wide = [t for t in valu if t.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32", "v_mad_u64_u32", "v_mad_i64_i32"))]
    return len(body), len(valu), len(lanes), len(f64), len(wide)


def main():
    fo, mo = parse(sys.argv[1])
    fn, mn = parse(sys.argv[2])
    want = sys.argv[3:]
    dem = demangle(sorted(mo))
    print("# kernel | old: resources, instructions valu lane-moves f64 wide-mul | new: the same")
    for k in mo:
        if k not in fo or not all(w in dem[k] for w in want):
            continue
        if k not in fn:
            print(f"{dem[k]} | {res(mo[k])} {counts(fo[k])} | MISSING")
            continue
        a, b = counts(fo[k]), counts(fn[k])
        print(f"{dem[k].split('(')[0]} | {res(mo[k])} insts={a[0]} valu={a[1]} lanes={a[2]} f64={a[3]} wmul={a[4]}"
              f" | {res(mn[k])} insts={b[0]} valu={b[1]} lanes={b[2]} f64={b[3]} wmul={b[4]}")


if __name__ == "__main__":
    main()
