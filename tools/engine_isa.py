#!/usr/bin/env python3
"""Static view of the chunked engine's code: compiles owgs_kernels.hip and owgs_engine_narrow.hip to gfx950 assembly
with the Makefile's flags and prints, per engine kernel instantiation, the static instruction count, the counts by
unit prefix (s_, v_, ds_, memory, other), the v_readlane / v_writelane sites (SGPR spill reloads / spills) and the
compiler's resource-usage remark (SGPRs, VGPRs, spills, scratch).  Needs hipcc, no GPU.

Each file is compiled three times: as the library builds it (both roles in one kernel), and with -DOWGS_ROLE_ONLY=0 /
=1, which fixes the kernels' role branch to the engine waves' / the I/O wave's body, so the two paths can be read apart.

    python tools/engine_isa.py [--src DIR] [--only-kernel SUBSTR] [--regions] > profiles/engine_split_isa.txt

--src points at another checkout's openwhisk_amd/ (a parent build, which ignores OWGS_ROLE_ONLY: its three rows are equal).

--regions compiles with -gline-tables-only as well and attributes every instruction of the two role builds to source
regions, twice: by the phase of the engine body it was inlined into (the outermost frame of its location: the body's
marker comments and a few anchor lines split it), and by the function its own line lies in (the innermost frame: the
inlined helpers).  Same columns per region; regions without instructions are left out.

--identity PARENT_PKG compares this tree with another checkout's openwhisk_amd/ instead (the check of a refactor): every
.hip file under csrc/ of both trees is compiled with the Makefile's flags for that file, and per kernel symbol the
instruction text (comments dropped, the function index of local labels normalised) and the .amdhsa_kernel descriptor
are compared.  One line per kernel: identical / differs, then the kernels only one tree has; identical kernels of the
libraries (rocprim instantiations) are only counted.
"""
import argparse
import concurrent.futures as cf
import difflib
import hashlib
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
    # (plain and target-specific assignments: "build/x.o build/y.o: ENGINEFLAGS := ...")
    for m in re.finditer(r"^(?:[^\n#=:]+:[ \t]*)?(\w+)[ \t]*[?:]?=[ \t]*(.*)$", text, re.M):
        var.setdefault(m.group(1), m.group(2).strip())
    def expand(s):
        for _ in range(4):
            s = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
        return s
    hipcc = os.environ.get("HIPCC", expand(var["HIPCC"]))
    return hipcc, expand(var["HIPFLAGS"]).split() + expand(var.get("ENGINEFLAGS", "")).split()


# lines of owgs_engine_body that start a region besides its marker comments (// ==== title, // ---- title)
BODY_ANCHORS = [
    (r"^\s+if \(sempty\) \{", "lanes' walks: start and choice"),
    (r"if \(maxc == 1 && pool_mode == 0\) \{", "lanes' walks: plain 4-step groups"),
    (r"if \(maxc > 1 && pool_mode == 0\) \{", "lanes' walks: concurrent 4-step groups"),
    (r"for \(int k = 0; k < KPROBE_G; \+\+k\) \{", "lanes' walks: general walk"),
    (r"bool done = mm >", "re-decisions: walk"),
    (r"if \(!done\) break;  // a long walk", "re-decisions: after the walk"),
    (r"if \(act && li >= l0 && li < l\) \{", "commit: decisions of lanes [f, l)"),
    (r"if \(act && li >= l\) \{", "commit: lanes from l on"),
]
BODY = "owgs_engine_body"


def source_regions(path):
    """(functions, phases) of one source file: functions = [(first line, last line, name)] of the definitions that
    start in column 0; phases = [(first line, title)] inside owgs_engine_body, in source order."""
    funcs, phases, cur = [], [], None
    for no, line in enumerate(open(path, errors="replace").read().splitlines(), 1):
        if cur is None:
            sig = re.sub(r"__launch_bounds__\([^)]*\)", "", line)
            m = re.match(r"^[A-Za-z_][^;#]*?\b(\w+)\s*\(", sig)
            if m and not re.match(r"^(typedef|struct|namespace|extern|static_assert|using|template|return|if|for|while)\b", line):
                if re.search(r"\{.*\}\s*(//.*)?$", line):
                    funcs.append((no, no, m.group(1)))  # a one-line definition
                elif not line.rstrip().endswith(";"):
                    cur = (no, m.group(1))
            continue
        if line.startswith("}"):
            funcs.append((cur[0], no, cur[1]))
            cur = None
            continue
        if cur[1] != BODY:
            continue
        m = re.match(r"^\s+// (?:={8,}|-{4,}) (.+)$", line)
        if m:
            phases.append((no, m.group(1).strip()[:56]))
            continue
        for pat, title in BODY_ANCHORS:
            if re.search(pat, line):
                phases.append((no, title))
    return funcs, phases


class Regions:
    def __init__(self, pkg):
        self.pkg, self.files = pkg, {}

    def _file(self, path):
        if path not in self.files:
            full = path if os.path.isabs(path) else os.path.join(self.pkg, path)
            self.files[path] = source_regions(full) if os.path.exists(full) and "/csrc/" in "/" + path else None
        return self.files[path]

    def func(self, path, line):
        f = self._file(path)
        if f is None:
            return "(runtime headers)"
        if line == 0:
            return "(compiler-generated)"
        for a, b, name in f[0]:
            if a <= line <= b:
                return name
        return os.path.basename(path)

    def phase(self, frames):
        """frames: innermost first.  The outermost frame inside owgs_engine_body names the phase; code outside the
        body goes by its outermost function (the kernel)."""
        path, line = frames[-1]
        for fr in reversed(frames):
            if self.func(*fr) == BODY:
                path, line = fr
                break
        name = self.func(path, line)
        if name != BODY:
            return name
        cur = "prologue"
        for no, title in self._file(path)[1]:
            if no > line:
                break
            cur = title
        return "body: " + cur


def compile_asm(pkg, src, extra, out):
    hipcc, flags = makefile_flags(pkg)
    # (run inside the package, so that the locations --regions reads name its files as csrc/NAME)
    cmd = [hipcc] + flags + extra + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                                     os.path.join("csrc", src)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=pkg)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"{src}: compile failed")
    return open(out).read(), r.stderr


def short_name(mangled):
    m = re.search(r"(owgs_engine(?:_multi_dev|_multi)?_kernel)ILi(\d+)E", mangled)
    if not m:
        return None
    return f"{m.group(1)}<{m.group(2)}>" + (" narrow" if "owgs_narrow" in mangled else "")


def new_counts():
    return dict(total=0, s=0, v=0, ds=0, mem=0, other=0, readlane=0, writelane=0)


def count_op(c, op):
    c["total"] += 1
    if op.startswith(MEM_PREFIXES):
        c["mem"] += 1
    elif op.startswith("s_"):
        c["s"] += 1
    elif op.startswith("v_"):
        c["v"] += 1
        c["readlane"] += op.startswith("v_readlane")
        c["writelane"] += op.startswith("v_writelane")
    elif op.startswith("ds_"):
        c["ds"] += 1
    else:
        c["other"] += 1


def parse_regions(text, reg):
    """{kernel: (by phase, by function)}: each instruction goes to the location of the last .loc before it, whose
    comment lists the inlining chain, innermost frame first: file:line:col @[ file:line:col @[ .. ] ]."""
    out, cur, loc, ph = {}, None, None, ""
    for line in text.splitlines():
        if cur is None:
            m = re.match(r"^(_Z\w+):", line)
            if m and short_name(m.group(1)):
                cur, loc, ph = short_name(m.group(1)), None, "(no location)"
                out[cur] = ({}, {})
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if re.match(r"^\s+\.loc\s", line):
            frames = re.findall(r"([^\s\[\]]+):(\d+):\d+", line.split(";", 1)[1]) if ";" in line else []
            loc = [(f, int(n)) for f, n in frames] or None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if not m:
            continue
        fn = reg.func(*loc[0]) if loc else "(no location)"
        # code without a line (spill code, merged instructions) goes with the phase of the located code before it
        if loc and loc[-1][1] != 0:
            ph = reg.phase(loc)
        count_op(out[cur][0].setdefault(ph, new_counts()), m.group(1))
        count_op(out[cur][1].setdefault(fn, new_counts()), m.group(1))
    return out


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


def file_flags(pkg):
    """(hipcc, flags of one csrc/NAME.hip as a function of NAME) from one reading of the Makefile: HIPFLAGS, plus
    ENGINEFLAGS for the files whose build/NAME.o is a target of the ENGINEFLAGS assignment."""
    hipcc, both = makefile_flags(pkg)
    m = re.search(r"^([^\n#=]+):[ \t]*ENGINEFLAGS[ \t]*:=[ \t]*(.*)$", open(os.path.join(pkg, "Makefile")).read(), re.M)
    targets, eng = (m.group(1).split(), m.group(2).split()) if m else ([], [])
    # makefile_flags returns HIPFLAGS followed by ENGINEFLAGS: the plain flags are that list without its tail
    assert both[len(both) - len(eng):] == eng, "ENGINEFLAGS is expected at the end of makefile_flags()"
    plain = both[:len(both) - len(eng)]
    return hipcc, lambda src: both if f"build/{os.path.splitext(src)[0]}.o" in targets else plain


def compile_one(pkg, hipcc, flags, src, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join("csrc", src)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=pkg)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"{src}: compile failed")
    return open(out).read()


def kernel_texts(asm):
    """{kernel symbol: (code lines, descriptor lines)}: the text between the symbol's label and its .Lfunc_end without
    comments, the function index in local labels dropped (.LBB<i>_<n> -> .LBB_<n>), and its .amdhsa_kernel block."""
    lines = asm.splitlines()
    desc, cur = {}, None
    for line in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = desc.setdefault(m.group(1), [])
        elif re.match(r"^\s*\.end_amdhsa_kernel", line):
            cur = None
        elif cur is not None:
            cur.append(" ".join(line.split(";", 1)[0].split()))
    out, cur = {}, None
    for line in lines:
        if cur is None:
            m = re.match(r"^(\w+):", line)
            if m and m.group(1) in desc:
                cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = " ".join(line.split(";", 1)[0].split())
        if t:
            cur.append(re.sub(r"(\.L[A-Za-z_]+)\d+_", r"\1_", t))
    return {k: (out.get(k, []), d) for k, d in desc.items()}


def identity(new_pkg, old_pkg):
    """Compare every kernel of every csrc/*.hip of two trees, each file compiled with its own tree's flags."""
    with tempfile.TemporaryDirectory() as d, cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        futs = []
        for side, pkg in (("new", new_pkg), ("parent", old_pkg)):
            hipcc, flags_of = file_flags(pkg)
            for src in sorted(f for f in os.listdir(os.path.join(pkg, "csrc")) if f.endswith(".hip")):
                futs.append((side, src, ex.submit(compile_one, pkg, hipcc, flags_of(src), src, os.path.join(d, f"{side}_{src}.s"))))
        found = {"new": {}, "parent": {}}
        for side, src, f in futs:
            for k, v in kernel_texts(f.result()).items():
                found[side].setdefault(k, []).append((src, v))
    # (library kernels are weak and instantiated in every file that uses them: a symbol found twice goes by file too)
    twice = {k for side in found for k, defs in found[side].items() if len(defs) > 1}
    kern = {side: {(f"{k} @{src}" if k in twice else k): (src, v) for k, defs in found[side].items() for src, v in defs}
            for side in found}
    def show(k):  # (library template instantiations run to a kilobyte: their head and a digest of the whole name)
        return k if len(k) <= 160 else f"{k[:120]}...#{hashlib.md5(k.encode()).hexdigest()[:8]}"
    n_same = n_diff = n_lib = 0
    for k in sorted(set(kern["new"]) & set(kern["parent"])):
        (sn, vn), (sp, vp) = kern["new"][k], kern["parent"][k]
        same = vn == vp
        n_same += same
        n_diff += not same
        if same and re.match(r"_ZN(7rocprim|6hipcub)", k):  # a library (rocprim) kernel: counted, listed only when it differs
            n_lib += 1
            continue
        what = "identical" if same else ("differs (code)" if vn[0] != vp[0] else "differs (descriptor)")
        if vn[0] != vp[0]:  # how far apart: lines on each side, and the lines a diff takes out of / puts into the parent's
            d = [x for x in difflib.unified_diff(vp[0], vn[0], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
            what += f" {len(vp[0])} -> {len(vn[0])} lines, -{sum(x[0] == '-' for x in d)} +{sum(x[0] == '+' for x in d)}"
        print(f"{what:22s} {show(k)}  [{sn}{'' if sn == sp else ' <- ' + sp}]")
    only_p = sorted(set(kern["parent"]) - set(kern["new"]))
    only_n = sorted(set(kern["new"]) - set(kern["parent"]))
    for k in only_p:
        print(f"{'parent only':22s} {show(k)}  [{kern['parent'][k][0]}]")
    for k in only_n:
        print(f"{'new only':22s} {show(k)}  [{kern['new'][k][0]}]")
    print(f"# {n_same} identical ({n_lib} of them library kernels, not listed), {n_diff} differ, {len(only_p)} parent only, "
          f"{len(only_n)} new only")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(HERE, "..", "openwhisk_amd"), help="the openwhisk_amd/ directory to read")
    ap.add_argument("--only-kernel", default="owgs_engine_kernel", help="substring of the kernels to print ('' = all three)")
    ap.add_argument("--regions", action="store_true", help="attribute the role builds' instructions to source regions")
    ap.add_argument("--identity", metavar="PARENT_PKG", help="compare every kernel's code with another checkout's openwhisk_amd/")
    a = ap.parse_args()
    pkg = os.path.abspath(a.src)
    if a.identity:
        return identity(pkg, os.path.abspath(a.identity))
    builds = [("both roles", []), ("engine waves", ["-DOWGS_ROLE_ONLY=0"]), ("I/O wave", ["-DOWGS_ROLE_ONLY=1"])]
    srcs = ["owgs_kernels.hip", "owgs_engine_narrow.hip"]
    extra_of = dict(builds)
    res, regs = {}, {}
    dbg = ["-gline-tables-only"] if a.regions else []
    with tempfile.TemporaryDirectory() as d, cf.ThreadPoolExecutor(max_workers=6) as ex:
        futs = {}
        for bi, (bname, extra) in enumerate(builds):
            for src in srcs:
                futs[ex.submit(compile_asm, pkg, src, extra + dbg, os.path.join(d, f"{bi}_{src}.s"))] = (bname, src)
        for f, (bname, src) in futs.items():
            asm, rem = f.result()
            counts, remarks = parse_asm(asm), parse_remarks(rem)
            if a.regions and extra_of[bname]:
                for k, r in parse_regions(asm, Regions(pkg)).items():
                    regs[(k, bname)] = r
            for k, c in counts.items():
                c.update(remarks.get(k, {}))
                res[(k, bname)] = c
    _, flags = makefile_flags(pkg)
    print("# flags: " + " ".join(flags + dbg))
    cols = ["total", "s", "v", "ds", "mem", "other", "readlane", "writelane", "sgpr", "sgpr_spill", "vgpr", "vgpr_spill",
            "scratch"]
    print(f"{'kernel':42s} {'build':13s} " + " ".join(f"{c:>10s}" for c in cols))
    for k in sorted({k for k, _ in res}):
        if a.only_kernel not in k:
            continue
        for bname, _ in builds:
            c = res[(k, bname)]
            print(f"{k:42s} {bname:13s} " + " ".join(f"{c.get(x, -1):>10d}" for x in cols))
    rcols = cols[:8]
    for (k, bname) in sorted(regs):
        if a.only_kernel not in k:
            continue
        for what, table in zip(("phase (outermost frame)", "function (innermost frame)"), regs[(k, bname)]):
            print(f"\n# {k}, {bname}: instructions by {what}")
            print(f"{'region':64s} " + " ".join(f"{c:>10s}" for c in rcols))
            for name, c in table.items():  # (first appearance in the code: roughly source order)
                print(f"{name:64s} " + " ".join(f"{c[x]:>10d}" for x in rcols))


if __name__ == "__main__":
    main()
