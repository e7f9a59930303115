"""Compare the gfx950 device code of HIP files between two trees of this repository, kernel by kernel.  Needs hipcc, no GPU.

    python tools/kernel_isa_diff.py TREE_A TREE_B fs_hyper.hip fs_plasticity.hip ...

Each file (a name under fenicssolver_amd/csrc) is compiled in both trees with the CXXFLAGS of that tree's csrc/Makefile plus
--cuda-device-only -S -Rpass-analysis=kernel-resource-usage, the assembly is split by kernel symbol, and per kernel one line says
  identical      every instruction equals the other side's, operands included (comments dropped, the numbers of local labels
                 normalised), or
  NOT identical  whether the sequence of fp64 opcodes (the mnemonics that contain "f64", in order) is equal, the VGPRs, scratch bytes
                 per lane and waves per SIMD of both sides, and the lines that differ (a unified diff of the instruction streams).
Kernels that only one side has are listed.  The exit status is 0 when every kernel of every file is identical and both sides have
the same kernels, 1 otherwise.  For a comparison with a commit, check that commit out next to the tree:
    git worktree add ../parent HEAD~1 && python tools/kernel_isa_diff.py ../parent . fs_hyper.hip
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("fenicssolver_amd", "csrc")


def makefile_flags(tree):
    """the CXXFLAGS of the tree's csrc/Makefile, $(ARCH) filled in"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_to_asm(tree, name, out):
    cmd = [os.environ.get("HIPCC", "hipcc")] + makefile_flags(tree) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                       "-o", out, name]
    p = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        sys.exit("%s failed in %s:\n%s" % (" ".join(cmd), tree, p.stderr[-4000:]))
    return open(out).read(), p.stderr


def resources(remarks):
    """{symbol: (VGPRs, scratch bytes per lane, waves per SIMD)} from the kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    return {k: (v.get("VGPRs"), v.get("ScratchSize"), v.get("Occupancy")) for k, v in out.items()}


def kernels(asm):
    """{symbol: [instruction, ...]} of every kernel (.amdhsa_kernel) of an assembly file"""
    lines = asm.splitlines()
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")]
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m:
            start.setdefault(m.group(1), i)
    out = {}
    for name in names:
        body = []
        for l in lines[start[name] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            text = l.split(";", 1)[0].strip()
            if not text or text.startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", text):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", text)))
        out[name] = body
    return out


def demangle(symbols):
    symbols = list(symbols)
    if not symbols:
        return {}
    try:
        p = subprocess.run(["c++filt"], input="\n".join(symbols) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True)
        names = p.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        names = symbols
    return {s: kernel_name(n) for s, n in zip(symbols, names)}


def kernel_name(demangled):
    """the function name with its template arguments: no return type, no "(anonymous namespace)::", no parameter list"""
    name = re.sub(r"^void ", "", demangled).replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(name):              # cut at the first '(' outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def fp64_sequence(body):
    return [i.split()[0] for i in body if not i.endswith(":") and "f64" in i.split()[0]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="+", help="file names under fenicssolver_amd/csrc")
    ap.add_argument("--max-diff-lines", type=int, default=40)
    args = ap.parse_args()
    all_same = True
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            side = []
            for tag, tree in (("a", args.tree_a), ("b", args.tree_b)):
                asm, remarks = compile_to_asm(os.path.abspath(tree), name, os.path.join(tmp, tag + ".s"))
                side.append((kernels(asm), resources(remarks)))
            (ka, ra), (kb, rb) = side
            pretty = demangle(set(ka) | set(kb))
            common = sorted(set(ka) & set(kb), key=lambda s: pretty[s])
            n_same = sum(ka[s] == kb[s] for s in common)
            print("== %s: %d kernels in A, %d in B, %d in both, %d of them identical instruction for instruction"
                  % (name, len(ka), len(kb), len(common), n_same))
            for tag, only in (("A", set(ka) - set(kb)), ("B", set(kb) - set(ka))):
                for s in sorted(only, key=lambda s: pretty[s]):
                    all_same = False
                    print("only in %s: %s" % (tag, pretty[s]))
            for s in common:
                a, b = ka[s], kb[s]
                n_inst = sum(not i.endswith(":") for i in a)
                if a == b:
                    print("%-72s identical (%d instructions, %d fp64)" % (pretty[s], n_inst, len(fp64_sequence(a))))
                    continue
                all_same = False
                fa, fb = fp64_sequence(a), fp64_sequence(b)
                print("%-72s NOT identical: fp64 opcode sequence %s (%d / %d) | VGPR %s -> %s | scratch %s -> %s B | waves/SIMD %s -> %s"
                      % (pretty[s], "equal" if fa == fb else "DIFFERS", len(fa), len(fb), ra.get(s, (None,) * 3)[0], rb.get(s, (None,) * 3)[0],
                         ra.get(s, (None,) * 3)[1], rb.get(s, (None,) * 3)[1], ra.get(s, (None,) * 3)[2], rb.get(s, (None,) * 3)[2]))
                diff = [l for l in difflib.unified_diff(a, b, "A", "B", lineterm="", n=0) if not l.startswith(("---", "+++"))]
                for l in diff[:args.max_diff_lines]:
                    print("    " + l)
                if len(diff) > args.max_diff_lines:
                    print("    ... %d more lines" % (len(diff) - args.max_diff_lines))
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
