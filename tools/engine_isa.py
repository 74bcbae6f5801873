#!/usr/bin/env python3
"""Static view of the chunked engine's code: compiles owgs_kernels.hip and owgs_engine_narrow.hip to gfx950 assembly
with the Makefile's flags and prints, per engine kernel instantiation, the static instruction count, the counts by
unit prefix (s_, v_, ds_, memory, other), the v_readlane / v_writelane sites (SGPR spill reloads / spills) and the
compiler's resource-usage remark (SGPRs, VGPRs, spills, scratch).  Needs hipcc, no GPU.

Each file is compiled three times: as the library builds it (both roles in one kernel), and with -DOWGS_ROLE_ONLY=0 /
=1, which fixes the kernels' role branch to the engine waves' / the I/O wave's body, so the two paths can be read apart.

    python tools/engine_isa.py [--src DIR] [--only-kernel SUBSTR] > profiles/engine_split_isa.txt

--src points at another checkout's openwhisk_amd/ (a parent build, which ignores OWGS_ROLE_ONLY: its three rows are equal).
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
MEM_PREFIXES = ("global_", "flat_", "buffer_", "scratch_", "s_load_", "s_buffer_load_")


def makefile_flags(pkg):
    """HIPCC, HIPFLAGS and ENGINEFLAGS as the Makefile sets them."""
    text = open(os.path.join(pkg, "Makefile")).read()
    var = {}
    for m in re.finditer(r"^(\w+)\s*[?:]?=\s*(.*)$", text, re.M):
        var.setdefault(m.group(1), m.group(2).strip())
    def expand(s):
        for _ in range(4):
            s = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
        return s
    hipcc = os.environ.get("HIPCC", expand(var["HIPCC"]))
    return hipcc, expand(var["HIPFLAGS"]).split() + expand(var.get("ENGINEFLAGS", "")).split()


def compile_asm(pkg, src, extra, out):
    hipcc, flags = makefile_flags(pkg)
    cmd = [hipcc] + flags + extra + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                                     os.path.join(pkg, "csrc", src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"{src}: compile failed")
    return open(out).read(), r.stderr


def short_name(mangled):
    m = re.search(r"(owgs_engine(?:_multi_dev|_multi)?_kernel)ILi(\d+)E", mangled)
    if not m:
        return None
    return f"{m.group(1)}<{m.group(2)}>" + (" narrow" if "owgs_narrow" in mangled else "")


def parse_asm(text):
    """{kernel: counts} for every engine kernel: instructions between the kernel's label and its .Lfunc_end."""
    out, cur = {}, None
    for line in text.splitlines():
        if cur is None:
            m = re.match(r"^(_Z\w+):", line)
            if m and short_name(m.group(1)):
                cur = dict(name=short_name(m.group(1)), total=0, s=0, v=0, ds=0, mem=0, other=0, readlane=0, writelane=0)
            continue
        if line.startswith(".Lfunc_end"):
            out[cur.pop("name")] = cur
            cur = None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if not m:
            continue  # labels, directives, comments
        op = m.group(1)
        cur["total"] += 1
        if op.startswith(MEM_PREFIXES):
            cur["mem"] += 1
        elif op.startswith("s_"):
            cur["s"] += 1
        elif op.startswith("v_"):
            cur["v"] += 1
            cur["readlane"] += op.startswith("v_readlane")
            cur["writelane"] += op.startswith("v_writelane")
        elif op.startswith("ds_"):
            cur["ds"] += 1
        else:
            cur["other"] += 1
    return out


def parse_remarks(text):
    out, cur = {}, None
    keys = {"SGPRs": "sgpr", "TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
            "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "Occupancy [waves/SIMD]": "occ"}
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = short_name(m.group(1))
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark: [^ ]* +([A-Za-z][^:]*): (\d+)", line)
        if m and cur and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(HERE, "..", "openwhisk_amd"), help="the openwhisk_amd/ directory to read")
    ap.add_argument("--only-kernel", default="owgs_engine_kernel", help="substring of the kernels to print ('' = all three)")
    a = ap.parse_args()
    pkg = os.path.abspath(a.src)
    builds = [("both roles", []), ("engine waves", ["-DOWGS_ROLE_ONLY=0"]), ("I/O wave", ["-DOWGS_ROLE_ONLY=1"])]
    srcs = ["owgs_kernels.hip", "owgs_engine_narrow.hip"]
    res = {}
    with tempfile.TemporaryDirectory() as d, cf.ThreadPoolExecutor(max_workers=6) as ex:
        futs = {}
        for bi, (bname, extra) in enumerate(builds):
            for src in srcs:
                futs[ex.submit(compile_asm, pkg, src, extra, os.path.join(d, f"{bi}_{src}.s"))] = (bname, src)
        for f, (bname, src) in futs.items():
            asm, rem = f.result()
            counts, remarks = parse_asm(asm), parse_remarks(rem)
            for k, c in counts.items():
                c.update(remarks.get(k, {}))
                res[(k, bname)] = c
    _, flags = makefile_flags(pkg)
    print("# flags: " + " ".join(flags))
    cols = ["total", "s", "v", "ds", "mem", "other", "readlane", "writelane", "sgpr", "sgpr_spill", "vgpr", "vgpr_spill",
            "scratch"]
    print(f"{'kernel':42s} {'build':13s} " + " ".join(f"{c:>10s}" for c in cols))
    for k in sorted({k for k, _ in res}):
        if a.only_kernel not in k:
            continue
        for bname, _ in builds:
            c = res[(k, bname)]
            print(f"{k:42s} {bname:13s} " + " ".join(f"{c.get(x, -1):>10d}" for x in cols))


if __name__ == "__main__":
    main()
