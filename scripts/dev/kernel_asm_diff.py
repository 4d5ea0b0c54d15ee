"""Compare the gfx950 kernels of two source trees instantiation by instantiation (no GPU needed).

    python scripts/dev/kernel_asm_diff.py OLD_CSRC NEW_CSRC old1.hip[,old2.hip...] new1.hip[,new2.hip...]

Compiles the named files of each tree to device assembly with the Makefile's flags, splits the assembly into
kernels, and prints for every kernel (demangled name) its VGPRs / SGPRs / scratch / static LDS / occupancy in both
trees and the number of instruction lines that differ (labels and comments stripped; 0 = the same instruction stream).
A kernel may move between files and may be renamed with --rename=OLD=NEW (substring of the demangled name);
--keep-old=DIR keeps the old tree's assembly in DIR and reuses it in the next run."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wall -Wno-unused-function -Wno-unused-command-line-argument".split()
EXTRA = {"syrk_bf16.hip": ["-fno-slp-vectorize"], "sparse_ent.hip": ["-Wno-inline-asm"]}
FIELDS = [("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
          ("lds", r"; LDSByteSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")]


def kernels(csrc, files, tmp):
    out = {}
    for f in files:
        s = os.path.join(tmp, f + ".s")
        if not os.path.exists(s):
            subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *EXTRA.get(f, []), "--cuda-device-only", "-S",
                                   os.path.join(csrc, f), "-o", s])
        text = open(s).read()
        for chunk in re.split(r"; -- Begin function ", text)[1:]:
            sym = chunk.split("\n", 1)[0].strip()
            if f".amdhsa_kernel {sym}\n" not in chunk:
                continue
            body, tail = re.split(r"^\.Lfunc_end\d+:\n", chunk.split(f"\n{sym}:", 1)[1], maxsplit=1, flags=re.M)
            ins = []
            for line in body.splitlines():
                line = line.split(";")[0].strip()
                if not line or line.startswith(".") or line.endswith(":"):
                    continue
                ins.append(re.sub(r"\.LBB\d+_\d+", ".LBB", line))
            res = {k: int(re.search(p, tail).group(1)) for k, p in FIELDS}
            out[sym] = (res, ins)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"^void ", "", n): v for n, v in zip(names, out.values())}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    keep = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--keep-old=")]   # reuse OLD's assembly there
    ren = [a.split("=", 2)[1:] for a in sys.argv[1:] if a.startswith("--rename=")]
    old_csrc, new_csrc, old_files, new_files = args
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        if keep:
            os.makedirs(keep[0], exist_ok=True)
        old = kernels(old_csrc, old_files.split(","), keep[0] if keep else t1)
        new = kernels(new_csrc, new_files.split(","), t2)
    for a, b in ren:
        old = {k.replace(a, b): v for k, v in old.items()}
    print(f"{'kernel':100s} {'vgpr':>9s} {'sgpr':>9s} {'scratch':>9s} {'lds':>11s} {'occ':>5s}  instr  differing")
    same = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name[:100]:100s} only in the {'old' if name in old else 'new'} tree")
            continue
        (ro, io), (rn, inn) = old[name], new[name]
        cols = " ".join(f"{str(ro[k]) + '/' + str(rn[k]):>{w}s}" for k, w in zip(ro, (9, 9, 9, 11, 5)))
        sm = difflib.SequenceMatcher(None, io, inn, autojunk=False)
        ndiff = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
        same += ndiff == 0
        print(f"{name[:100]:100s} {cols}  {len(io):5d}/{len(inn):<5d} {ndiff}")
    print(f"{same} of {len(set(old) | set(new))} kernels compile to the same instruction stream")


if __name__ == "__main__":
    main()
