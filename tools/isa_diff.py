"""Is the gfx950 code of every kernel the same in two trees?   python tools/isa_diff.py OLD_TREE NEW_TREE [-j N]

For every .hip of SRCS in eabnet_amd/csrc/Makefile, each tree's device assembly is built with that tree's own HIPCC, ARCH and FLAGS
(asked of make, not restated here; -save-temps gives way to --cuda-device-only -S).  Per kernel it compares the instruction sequence
(comments stripped, mangled names reduced to their base names) and the figures of the kernel's metadata: VGPRs, AGPRs, SGPRs, LDS
bytes, scratch bytes.  Other assembler directives and the __hip_cuid_* label are ignored.  A kernel is matched by its base name
(demangled, without the parameter list) and its position among the kernels of that name in the file, so a renamed parameter type
does not unmatch it.  A kernel whose metadata lacks one of the five figures is an error, not a match.  One line per kernel: `same`,
or the first differing lines; the exit status is 1 on any difference.
It is a diff and nothing else: the rule for a refactor that is meant to leave the kernels alone."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
SYMBOL = re.compile(r"\b_Z[\w.$]+")


def make_vars(csrc):
    """HIPCC, ARCH, FLAGS and SRCS as csrc/Makefile expands them."""
    names = ("HIPCC", "ARCH", "FLAGS", "SRCS")
    rule = "isa-diff-vars: ; @" + " ; ".join(f"echo '$({n})'" for n in names)
    r = subprocess.run(["make", "-s", "-C", csrc, "-f", "Makefile", "--no-print-directory", "--eval", rule, "isa-diff-vars"],
                       capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def assemble(csrc, v, src, out):
    flags = [f for f in v["FLAGS"].split() if not f.startswith("-save-temps")]
    r = subprocess.run([v["HIPCC"], *flags, "--cuda-device-only", "-S", src, "-o", out], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{os.path.join(csrc, src)} does not compile:\n{r.stderr[-4000:]}")


def base_names(symbols):
    """mangled -> demangled name without its parameter list ('void k<true, 4>(float const*)' -> 'k<true, 4>')"""
    symbols = sorted(symbols)
    if not symbols:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.splitlines()
    names = {}
    for sym, dn in zip(symbols, out):
        if dn.endswith(")"):                                 # cut the last balanced (...)
            depth = 0
            for i in range(len(dn) - 1, -1, -1):
                depth += (dn[i] == ")") - (dn[i] == "(")
                if depth == 0:
                    dn = dn[:i]
                    break
        names[sym] = dn.split(" ", 1)[1] if dn.startswith("void ") else dn
    return names


def kernels(path):
    """[(base name, occurrence), instruction lines, figures] of every kernel of an assembly file, in file order"""
    lines = open(path).read().splitlines()
    names = base_names(set(SYMBOL.findall("\n".join(lines))))
    figures, cur, item = {}, None, None
    for ln in lines:                                         # the entries of the metadata's amdhsa.kernels list
        if item is None:
            if ln.strip() == "amdhsa.kernels:":
                item = ""
            continue
        if item == "":                                       # the list's own indentation: that of its first '- '
            item = re.match(r" *- ", ln).group(0)
        if not ln.startswith(" " * len(item)) and not ln.startswith(item):
            break                                            # the next top-level key ends the list
        if ln.startswith(item):                              # '- .agpr_count' at the list's indentation opens a kernel;
            cur = {}                                         # the '- ' items of its .args are nested deeper
        m = re.match(r"(\.\w+): *(.*)", ln[len(item):])      # a key of the entry itself, not of a nested item
        if m and m.group(1) in FIGURES:
            cur[m.group(1)] = m.group(2)
        elif m and m.group(1) == ".name":
            figures[m.group(2)] = cur
    is_kernel = {ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")}
    for sym in sorted(is_kernel):                            # a figure that was not found would compare equal to itself
        missing = [k for k in FIGURES if k not in figures.get(sym, {})]
        if missing:
            sys.exit(f"{path}: no {', '.join(missing)} in the metadata of {sym}")
    found, seen, body, sym = [], {}, None, None
    for ln in lines:
        m = re.match(r"([\w.$]+):", ln)
        if body is None:
            if m and m.group(1) in is_kernel:
                sym, body = m.group(1), []
            continue
        if ln.startswith(".Lfunc_end"):
            key = names.get(sym, sym)
            seen[key] = seen.get(key, 0) + 1
            found.append(((key, seen[key]), body, figures[sym]))
            body = None
            continue
        s = ln.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.endswith(":")):   # blank, comment or directive; labels stay
            continue
        s = SYMBOL.sub(lambda t: names.get(t.group(0), t.group(0)), s)
        body.append(re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", s))     # the function's number in a local label
    return found


def compare(src, old_s, new_s):
    old, new = kernels(old_s), kernels(new_s)
    new_by_key = {k: (b, f) for k, b, f in new}
    differs = 0
    for key, body, fig in old:
        label = f"{src}: {key[0]}" + (f" #{key[1]}" if key[1] > 1 else "")
        if key not in new_by_key:
            print(f"{label}: only in OLD_TREE")
            differs += 1
            continue
        nbody, nfig = new_by_key.pop(key)
        if body == nbody and fig == nfig:
            print(f"{label}: same")
            continue
        differs += 1
        print(f"{label}: DIFFERS")
        for k in FIGURES:
            if fig.get(k) != nfig.get(k):
                print(f"    {k} {fig.get(k)} -> {nfig.get(k)}")
        for d in list(difflib.unified_diff(body, nbody, "old", "new", n=1, lineterm=""))[2:14]:
            print("    " + d)
    for key in new_by_key:
        print(f"{src}: {key[0]}: only in NEW_TREE")
        differs += 1
    return len(old), differs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compilations at a time")
    a = ap.parse_args()
    csrc = [os.path.join(os.path.abspath(t), "eabnet_amd", "csrc") for t in (a.old_tree, a.new_tree)]
    v = [make_vars(c) for c in csrc]
    if v[0]["SRCS"].split() != v[1]["SRCS"].split():
        print(f"SRCS differ: {v[0]['SRCS']} -> {v[1]['SRCS']}")
    srcs = [s for s in v[0]["SRCS"].split() if s in v[1]["SRCS"].split()]
    total = differs = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        jobs = [pool.submit(assemble, csrc[side], v[side], s, os.path.join(tmp, f"{side}_{s}.s")) for s in srcs for side in (0, 1)]
        for j in jobs:
            j.result()
        for s in srcs:
            n, d = compare(s, os.path.join(tmp, f"0_{s}.s"), os.path.join(tmp, f"1_{s}.s"))
            total, differs = total + n, differs + d
    differs += v[0]["SRCS"].split() != v[1]["SRCS"].split()
    print(f"{total} kernels in {len(srcs)} files, {differs} differ" if differs else f"{total} kernels in {len(srcs)} files: all same")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
