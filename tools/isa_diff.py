"""Which kernels of the library differ between two builds of its device code (no GPU needed):
    python tools/isa_diff.py before.s after.s          (the files of `tools/isa_kernel.py build`, or of the same hipcc line without -gline-tables-only)
One line per kernel whose instruction stream differs -- instruction lines only: labels, directives and comments are dropped, the function index in the
names of local labels too --, with the number of instructions, vgpr_count, sgpr_count and scratch bytes on both sides; kernels that only one file has;
then the number of kernels that are identical."""
import re, subprocess, sys


def kernels(path):
    """-> {mangled name: ([instruction lines], {metadata})}"""
    txt = open(path).read()
    meta = {}
    for k in re.findall(r"- \.agpr_count.*?(?=\n  - \.agpr_count|\namdhsa\.target)", txt, flags=re.S):
        g = lambda key: (re.search(r"\." + key + r":\s*(\S+)", k) or [None, None])[1]
        meta[g("name")] = {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size")}
    out, name, body = {}, None, []
    for ln in txt.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name], name = (body, meta[name]), None
            continue
        s = re.sub(r"\s+", " ", ln.split(";")[0].split("//")[0]).strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
names = sorted(set(a) | set(b))
shown = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")))
same = 0
for n in names:
    d = shown[n].replace("(anonymous namespace)::", "").replace("void ", "")
    d = re.sub(r"\(.*\)$", "", d)[:110]
    if n not in a or n not in b:
        print(f"{d}: only in {sys.argv[2] if n in b else sys.argv[1]}")
    elif a[n][0] == b[n][0]:
        same += 1
    else:
        (ia, ma), (ib, mb) = a[n], b[n]
        print(f"{d}: instructions {len(ia)} -> {len(ib)}, vgpr {ma['vgpr']} -> {mb['vgpr']}, sgpr {ma['sgpr']} -> {mb['sgpr']}, scratch {ma['scratch']} -> {mb['scratch']}")
print(f"{same} of {len(names)} kernels identical")
