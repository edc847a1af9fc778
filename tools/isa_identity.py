"""Do two checkouts compile to the same gfx950 device code?  For a refactor that must not change a kernel: every
csrc/*.hip file is compiled device-only to assembly in both trees, with the flags csrc/Makefile gives that file
(CXXFLAGS and CXXFLAGS_<stem>), and the two listings are compared kernel by kernel after dropping what cannot affect
execution (comments, blank lines, .file / .ident, the hash in the __hip_cuid_ symbol).  A kernel is its instruction sequence plus its .amdhsa_kernel
resource block (VGPRs, SGPRs, LDS, scratch); everything outside the functions (LDS symbols, the metadata note) is one
more row, "(rest of file)".  CPU only: needs hipcc, no GPU.  It compares two builds and inspects nothing else.

    python tools/isa_identity.py --tree OTHER_CHECKOUT [--ablation] [--jobs N] [--diff N] [files ...]

files: names under csrc/ (conv_pipe.hip ...); default: every .hip file whose text differs between the trees, or all of
them when a csrc/*.h header differs.  --ablation adds the flag of `make ABLATION=1`; --diff N prints the first N lines
of each difference.  Prints, per file and kernel, the instruction count and identical / DIFFERS; exit status 1 on any
difference."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "explaining-in-style-reproducibility-study_amd"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_flags(csrc, stem, ablation):
    """CXXFLAGS + CXXFLAGS_<stem> of csrc/Makefile, with $(ARCH) filled in; warnings flags are left out."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    flags = [f for f in flags if not f.startswith("-W")]
    extra = re.search(r"^CXXFLAGS_%s\s*=\s*(.*)$" % re.escape(stem), text, re.M)
    if extra:
        flags += extra.group(1).split()
    if ablation:
        flags.append("-DSTYLEX_PIPE_ABLATION")
    return flags


def compile_asm(csrc, src, out, ablation):
    cmd = [HIPCC] + makefile_flags(csrc, src[:-4], ablation) + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return out


def split_asm(path):
    """{function name: [lines]} with the .amdhsa_kernel block appended to its kernel, and the rest under None."""
    parts, cur, rest = {}, None, []
    for raw in open(path):
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", raw.split(";", 1)[0].rstrip())  # a hash of the source text
        if not line.strip() or re.match(r"\s*\.(file|ident)\b", line):
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m or k:
            cur = (m or k).group(1)
            parts.setdefault(cur, [])
        (parts[cur] if cur else rest).append(line)
        if re.match(r"\s*\.size\s+%s," % re.escape(cur or "\0"), line) or re.match(r"\s*\.end_amdhsa_kernel", line):
            cur = None
    parts[None] = rest
    return parts


def n_instructions(lines):
    return sum(1 for l in lines if not re.match(r"\s*(\.|\S+:)", l))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", required=True, help="root of the checkout to compare with")
    ap.add_argument("--ablation", action="store_true", help="compile with -DSTYLEX_PIPE_ABLATION (make ABLATION=1)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--diff", type=int, default=0, metavar="N", help="print the first N lines of each difference")
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    new, old = os.path.join(HERE, PKG, "csrc"), os.path.join(os.path.abspath(args.tree), PKG, "csrc")

    def text(d, f):
        p = os.path.join(d, f)
        return open(p).read() if os.path.isfile(p) else None

    files = args.files
    if not files:
        hips = sorted(f for f in os.listdir(new) if f.endswith(".hip"))
        heads = sorted(set(f for d in (new, old) for f in os.listdir(d) if f.endswith(".h")))
        if any(text(new, h) != text(old, h) for h in heads):
            files = hips
        else:
            files = [f for f in hips if text(new, f) != text(old, f)]
    missing = [f for f in files if text(old, f) is None or text(new, f) is None]
    if missing:
        sys.exit("not in both trees: %s" % " ".join(missing))

    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.jobs) as pool:
        jobs = [(f, pool.submit(compile_asm, new, f, os.path.join(tmp, "new_" + f + ".s"), args.ablation),
                 pool.submit(compile_asm, old, f, os.path.join(tmp, "old_" + f + ".s"), args.ablation)) for f in files]
        for f, a, b in jobs:
            pa, pb = split_asm(a.result()), split_asm(b.result())
            print("%s%s" % (f, "  (ABLATION=1)" if args.ablation else ""))
            for name in sorted(set(pa) | set(pb), key=lambda n: (n is None, n or "")):
                la, lb = pa.get(name), pb.get(name)
                same = la == lb
                bad += not same
                label = name or "(rest of file)"
                if la is None or lb is None:
                    print("  %-9s %s  only in the %s tree" % ("DIFFERS", label, "other" if la is None else "new"))
                else:
                    count = "%6d" % n_instructions(la) if same else "%6d/%d" % (n_instructions(la), n_instructions(lb))
                    print("  %-9s %s instr  %s" % ("identical" if same else "DIFFERS", count, label))
                    if not same and args.diff:
                        d = difflib.unified_diff(lb, la, "other", "new", n=1, lineterm="")
                        print("\n".join("      " + l for l in list(d)[:args.diff]))
    print("%d file(s): %s" % (len(files), "all identical" if not bad else "%d DIFFERENCE(S)" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
