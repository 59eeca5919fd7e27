#!/usr/bin/env python3
"""Compare the device assembly of one .hip file from two trees: `hipcc <build.sh's flags> --cuda-device-only -S f.hip -o X.s` in each.
usage: device_asm_compare.py A.s B.s [A2.s B2.s ...]      exit status 1 when any pair differs in a kernel

Per pair: the whole-file diff behind the filter of profiles/neuron_host_dispatch_device_code.txt (the lines that carry only a path hash
or the compiler's name), then - for a host-side change that makes hipcc emit the same kernels in another ORDER - the comparison kernel
by kernel: the text of every function, its .amdhsa_kernel descriptor and its metadata entry, keyed by symbol.  What depends on a
function's position in the file is normalised first: the function index in local labels and in the loop comments (.LBB<i>_<n>,
BB<i>_<n>, .Lfunc_end<i>, .Ltmp<n>) and the column the comments start in (it follows the label's width)."""
import difflib
import re
import sys

DROP = re.compile(r"__hip_cuid_|^\s*\.file|^\s*\.ident")


def load(path):
    return [line.rstrip("\n") for line in open(path) if not DROP.search(line)]


def norm(line):
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
    line = re.sub(r"\bBB\d+_", "BB_", line)
    return re.sub(r"\s+;", " ;", line)


def pieces(lines):
    """(function texts, kernel descriptors, metadata entries), each {symbol: lines}; the descriptors keep the file's kernel order"""
    text, desc, meta = {}, {}, {}
    cur = name = None
    for line in lines:
        m = re.match(r"^\s*\.type\s+([^,]+),@function", line)
        if m:
            name, cur = m.group(1), []
        if cur is not None:
            cur.append(norm(line))
            if re.match(r"^\.Lfunc_end\d+:", line):
                text[name], cur = cur, None
    cur = name = None
    for line in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), []
        if cur is not None:
            cur.append(line)
            if re.match(r"^\s*\.end_amdhsa_kernel", line):
                desc[name], cur = cur, None
    cur = name = None
    inside = False
    for line in lines:
        if ".amdgpu_metadata" in line:
            inside = not inside
        if not inside:
            continue
        if re.match(r"^\s+- \.(agpr_count|args):", line) or line.startswith("amdhsa.target"):      # next entry / the trailer
            if cur is not None and name:
                meta[name] = cur
            cur, name = ([], None) if not line.startswith("amdhsa.target") else (None, None)
        if cur is not None:
            m = re.match(r"^\s+\.symbol:\s+(\S+)", line)
            if m:
                name = m.group(1)
            cur.append(line)
    return text, desc, meta


bad = 0
for pa, pb in zip(sys.argv[1::2], sys.argv[2::2]):
    a, b = load(pa), load(pb)
    whole = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
    A, B = pieces(a), pieces(b)
    same_set = all(sorted(x) == sorted(y) for x, y in zip(A, B))
    differing = sum(1 for x, y in zip(A, B) for k in set(x) | set(y) if x.get(k) != y.get(k))
    assert len(A[0]) == len(A[1]) == len(A[2]) > 0, "a kernel without text, descriptor or metadata entry: the splitter missed something"
    print(f"{pb}: {len(b)} asm lines, {len(B[1])} kernels; whole-file diff {whole} lines; same kernel set: {same_set}; "
          f"same order: {list(A[1]) == list(B[1])}; kernels that differ in text, descriptor or metadata: {differing}")
    bad += differing + (not same_set)
sys.exit(1 if bad else 0)
