"""Dev tool: do two trees compile to the same kernels?  `kernel_isa.py A B [--flavour release|dev]`: A and B are checkouts (every
unit of icpslam_amd/csrc is compiled to device assembly with the Makefile's own command lines for that flavour) or directories of
`hipcc --cuda-device-only -S` output.  Per kernel symbol it compares the code between the kernel's label and its end marker -- with
per-function label numbers normalised and trailing comments stripped -- and the .amdhsa_kernel resource block (registers, LDS,
scratch), and prints `same` or `different`.  It only compares two texts.  Exit status 1 if any kernel differs or is missing."""
import argparse, concurrent.futures, glob, os, re, shlex, subprocess, sys, tempfile

# labels numbered per function or per unit: the numbers follow a kernel's place in its unit, not its code
LABELS = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"), (re.compile(r"\.Lfunc_([a-z]+)\d+"), r".Lfunc_\1"),
          (re.compile(r"\.Lpost_getpc\d+"), ".Lpost_getpc")]


def assemble(tree, flavour, out):
    """the Makefile's compile line of every kernel unit, with the device assembly as its only product"""
    csrc = os.path.join(tree, "icpslam_amd", "csrc")
    target = "../libicpgpu_dev.so" if flavour == "dev" else "../libicpgpu.so"
    plan = subprocess.run(["make", "-C", csrc, "-n", "-B", "FLAVOUR=" + flavour, target], capture_output=True, text=True, check=True).stdout
    jobs = []
    for line in plan.splitlines():
        words = shlex.split(line)
        if "-c" not in words or not words[words.index("-c") + 1].endswith(".hip"):
            continue
        unit = words[words.index("-c") + 1]
        keep = [w for w in words[: words.index("-c")] if w not in ("-MMD", "-MP")]
        jobs.append(keep + ["--cuda-device-only", "-S", unit, "-o", os.path.join(out, unit + ".s")])
    with concurrent.futures.ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        for r in pool.map(lambda j: subprocess.run(j, cwd=csrc, capture_output=True, text=True), jobs):
            if r.returncode:
                sys.exit(r.stderr)


def kernels(path, flavour):
    """{symbol: (code, resource block)} of every kernel under `path`"""
    tmp = None
    if os.path.exists(os.path.join(path, "icpslam_amd", "csrc", "Makefile")):
        tmp = tempfile.TemporaryDirectory()
        assemble(path, flavour, tmp.name)
        path = tmp.name
    found = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))):
        lines = [l.rstrip("\n") for l in open(f)]
        for i, l in enumerate(lines):
            if not l.lstrip().startswith(".amdhsa_kernel "):
                continue
            sym = l.split()[1]
            j = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
            res = "\n".join(x.strip() for x in lines[i:j])
            a = next(k for k in range(len(lines)) if lines[k].startswith(sym + ":"))
            b = next(k for k in range(a, len(lines)) if lines[k].startswith(".Lfunc_end"))
            code = []
            for x in lines[a + 1 : i] + lines[j + 1 : b]:
                x = x.split(";")[0].rstrip()
                for pat, to in LABELS:
                    x = pat.sub(to, x)
                if x:
                    code.append(x)
            found[sym] = ("\n".join(code), res)
    return found


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--flavour", default="release", choices=("release", "dev"))
    args = ap.parse_args()
    ka, kb = kernels(args.a, args.flavour), kernels(args.b, args.flavour)
    same = 0
    for sym in sorted(set(ka) | set(kb)):
        if sym not in ka or sym not in kb:
            verdict = "only in " + (args.a if sym in ka else args.b)
        elif ka[sym] == kb[sym]:
            verdict, same = "same", same + 1
        else:
            verdict = "different (" + ", ".join(n for n, k in (("code", 0), ("resources", 1)) if ka[sym][k] != kb[sym][k]) + ")"
        print(f"{verdict:24s} {sym}")
    print(f"{len(set(ka) | set(kb))} kernels compared, {same} identical")
    sys.exit(0 if same == len(set(ka) | set(kb)) else 1)
