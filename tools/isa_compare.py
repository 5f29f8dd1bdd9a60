"""Compare the device code of two `hipcc -S --offload-device-only` listings function by function.

  python tools/isa_compare.py OLD_DIR NEW_DIR mapf_fused mapf_rollout_wide ... > profiles/<name>.txt

For every function of OLD_DIR/<src>.s (kernels and non-inlined device functions) the function of
NEW_DIR/<src>.s with the same name is found -- the same demangled name once `false` / `true` read 0 / 1
(a bool template parameter that became an int) and allowing one or two defaulted parameters (0) appended
to the template list -- and their instruction text compared after removing assembler comments, symbol
names and the function index of .LBB<n>_<m> labels.  Kernels' resources (.vgpr_count,
.sgpr_spill_count, .private_segment_fixed_size) come from the metadata and must be equal too.  New
functions without a counterpart are listed with their resources.  Exit status 1 if any differ.
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def key_of(dem):
    return re.sub(r"\bfalse\b", "0", re.sub(r"\btrue\b", "1", dem))


def with_defaults(key, k):
    """key with k defaulted `0` template arguments appended to the function's own template list."""
    i = key.find(">(")
    return key if i < 0 else key[:i] + ", 0" * k + key[i:]


def parse(path):
    funcs, meta = {}, {}
    names = set()
    lines = open(path).read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            names.add(m.group(1))
    cur, body = None, []
    for ln in lines:
        m = re.match(r"^(\S+):", ln)
        if cur is None and m and m.group(1) in names:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                funcs[cur] = body
                cur = None
                continue
            t = ln.split(";")[0].strip()
            if not t:
                continue
            t = re.sub(r"_Z\w+", "SYM", t)
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            body.append(t)
    name = None
    for ln in lines:
        m = re.match(r"\s*\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
            meta.setdefault(name, {})
        m = re.match(r"\s*\.(vgpr_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and name:
            meta[name][m.group(1)] = int(m.group(2))
    return funcs, meta


def res(m):
    return "vgprs=%s sgpr_spills=%s scratch=%s" % (m.get("vgpr_count", "-"), m.get("sgpr_spill_count", "-"),
                                                    m.get("private_segment_fixed_size", "-"))


def main():
    old_dir, new_dir, srcs = sys.argv[1], sys.argv[2], sys.argv[3:]
    total = same = 0
    added = []
    print("# Device code before and after, per function: instruction text between the label and .Lfunc_end")
    print("# without comments, symbol names and .LBB function indices; kernels' metadata resources.")
    print("# One line per function of the old listing: old name, new name, resources (new), identical yes / NO.")
    for src in srcs:
        fo, mo = parse(f"{old_dir}/{src}.s")
        fn, mn = parse(f"{new_dir}/{src}.s")
        do, dn = demangle(sorted(fo)), demangle(sorted(fn))
        by_key = {key_of(d): n for n, d in dn.items()}
        used = set()
        print(f"# {src}.hip: {len(fo)} functions before, {len(fn)} after")
        for o in sorted(fo):
            k = key_of(do[o])
            n = next((by_key[c] for c in (k, with_defaults(k, 1), with_defaults(k, 2)) if c in by_key), None)
            total += 1
            if n is None:
                print(f"{o} MISSING identical=NO")
                continue
            used.add(n)
            ok = fo[o] == fn[n] and mo.get(o, {}) == mn.get(n, {})
            same += ok
            print(f"{o} {n} {res(mn.get(n, {}))} instructions={len(fn[n])} identical={'yes' if ok else 'NO'}")
        added += [(src, n, mn.get(n, {}), len(fn[n])) for n in sorted(fn) if n not in used]
    print(f"# {total} functions compared, {same} identical, {total - same} differing")
    print(f"# {len(added)} new functions (no counterpart before):")
    for src, n, m, k in added:
        print(f"{src}: {n} {res(m)} instructions={k}")
    return 0 if total == same else 1


if __name__ == "__main__":
    sys.exit(main())
