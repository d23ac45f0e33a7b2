"""Compare the kernels of one .hip file between two builds: the compiler's -Rpass-analysis=kernel-resource-usage lines and the
code length of every kernel symbol.  No GPU.

For each build: compile with
    hipcc --offload-arch=gfx950 <the flags of build.py> -Rpass-analysis=kernel-resource-usage -c FILE.hip -o X.o 2> X_raw.txt
take the gfx950 code object out of X.o (llvm-objcopy --only-section=.hip_fatbin, clang-offload-bundler --unbundle) and list its
function symbols with `llvm-readelf -sW X.elf | awk '$4=="FUNC"{print $3, $8}' > X_sizes.txt`.  Then
    python tools/resource_usage_diff.py PARENT_raw.txt PARENT_sizes.txt THIS_raw.txt THIS_sizes.txt > resource_usage.txt
"""
import re
import subprocess
import sys

COLS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "SGPRs Spill", "VGPRs Spill"]
PAT = re.compile(r"remark:\s+(Function Name|" + "|".join(re.escape(c) for c in COLS) + r"): (\S+)")


def parse(raw, sizes):
    size = {}
    with open(sizes) as f:
        for ln in f:
            n, name = ln.split()
            size[name] = int(n)
    rows, cur = {}, None
    with open(raw) as f:
        for ln in f:
            m = PAT.search(ln)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = m.group(2)
                rows[cur] = {}
            else:
                rows[cur][m.group(1)] = m.group(2)
    names = list(rows) + [m for m in size if m not in rows]      # the latter: out-of-line device functions (no remark, a length only)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {p: (rows[m], size.get(m)) for m, p in zip(names, plain) if m in rows}, {p: size[m] for m, p in zip(names, plain) if m not in rows}


def fmt(entry):
    r, s = entry
    return " ".join(f"{r.get(c, '?'):>5}" for c in COLS) + f" {s if s is not None else '?':>7}"


def main():
    (parent, parent_fn), (this, this_fn) = parse(sys.argv[1], sys.argv[2]), parse(sys.argv[3], sys.argv[4])
    same = sum(name in this and fmt(parent[name]) == fmt(this[name]) for name in parent)
    print("columns: SGPRs VGPRs AGPRs scratch[B/lane] occupancy[waves/SIMD] static-LDS[B/block] SGPR-spill VGPR-spill code[bytes]")
    print(f"summary: {len(parent)} kernels at the parent commit, {same} with identical lines and code length at this one, "
          f"{len(parent) - same} that differ; {len(set(this) - set(parent))} new kernels\n")
    print("== kernels of the parent commit ==")
    for name in sorted(parent):
        a, b = fmt(parent[name]), (fmt(this[name]) if name in this else "(gone)")
        print(f"{name}\n    parent {a}\n    this   {b}   {'same' if a == b else 'DIFFERS'}")
    print("\n== kernels new at this commit ==")
    for name in sorted(set(this) - set(parent)):
        print(f"{name}\n    this   {fmt(this[name])}")
    print("\n== out-of-line device functions (the compiler prints no remark for them): code[bytes] parent | this ==")
    for name in sorted(set(parent_fn) | set(this_fn)):
        a, b = parent_fn.get(name), this_fn.get(name)
        print(f"{name}\n    {a if a is not None else '-':>7} {b if b is not None else '-':>7}   {'same' if a == b else ('new' if a is None else 'DIFFERS')}")


if __name__ == "__main__":
    main()
