"""The code of the headline kernel (k_admm_solve_d<12, 4, 50, true, 4, 25, false>, the plain 16-lane quadrotor N=50 kernel) as the
build produced it: sha256 over its instructions (labels renumbered, comments and directives dropped), plus the compiler's version.
The kernel's speed depends on details of the generated code that no source-level reasoning predicts (+-2.5 % between builds with the
same instruction mix: profiles/r03_dgroup_ab.txt), so a change of this hash means: run tools/headline_ab.py against the previous
build on ONE box before believing any number, then record the new hash.
Each measured state has a record of its own under tests/golden/ (headline_kernel_code*.json); RECORD names the current one. A record
is never rewritten: a change that moves the headline's code adds a new file, points RECORD at it and records there.
The lean form of the same kernel (k_admm_solve_d_lean<12, 4, 50, true, 4, 25>, tinympc_lean_d.hip: what the headline runs since its
sweeps dropped the residual maxima nothing reads) has a record of its own, RECORD_LEAN, with the same rules.
    python tools/headline_code_hash.py                 print the hashes of the current build
    python tools/headline_code_hash.py --record        write RECORD (after the A/B)
The lean kernel with its accumulator starts read from LDS and its loop control hoisted (k_admm_solve_d_lean_start<12, 4, 50, true, 4, 25>,
tinympc_lstart_d.hip: what the headline runs now) has the third, RECORD_LEAN_START.
    python tools/headline_code_hash.py --record-lean   write RECORD_LEAN (after the A/B)
    python tools/headline_code_hash.py --record-lean-start   write RECORD_LEAN_START (after the A/B)
The lean-start kernel with the d stores of its lean rounds going through a per-lane address instead of a narrowed EXEC
(k_admm_solve_d_lean_trim<12, 4, 50, true, 4, 25>, tinympc_ltrim_d.hip: what the headline runs now) has the fourth, RECORD_LEAN_TRIM.
    python tools/headline_code_hash.py --record-lean-trim    write RECORD_LEAN_TRIM (after the A/B)
The trimmed kernel with d and the slack sharing the register slots inside a run of lean rounds (k_admm_solve_d_lean_share<12, 4, 50, true, 4, 25>,
tinympc_lshare_d.hip: what the headline runs now) has the fifth, RECORD_LEAN_SHARE.
    python tools/headline_code_hash.py --record-lean-share   write RECORD_LEAN_SHARE (after the A/B)
The shared kernel with twelve LDS slots turned into register slots inside a run of lean rounds (k_admm_solve_d_lean_park<12, 4, 50, true, 4, 25>,
tinympc_lpark_d.hip: what the headline runs now) has the sixth, RECORD_LEAN_PARK.
    python tools/headline_code_hash.py --record-lean-park    write RECORD_LEAN_PARK (after the A/B)"""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN7tinympc14k_admm_solve_dILi12ELi4ELi50ELb1ELi4ELi25ELb0EEEvNS_11SolveParamsE"
# the current record (the earlier ones stay as the history of measured states: headline_kernel_code.json, the build before knot 0
# and the backward tail were folded out of the sweeps)
RECORD = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_fold.json")
KERNEL_LEAN = "_ZN7tinympc19k_admm_solve_d_leanILi12ELi4ELi50ELb1ELi4ELi25EEEvNS_11SolveParamsE"
SOURCE_LEAN = "tinympc_lean_d.hip"
RECORD_LEAN = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_lean.json")
# what was measured for the lean kernel's recorded code (profiles/d_lean_headline_ab.txt)
LEAN_MEASURED = ("kernel 1.436 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_lean_kernel_stats.csv); tools/headline_ab.py, one box, against "
                 "the parent build's plain kernel (4,249 instructions, headline_kernel_code_d_fold.json): 1.4326 vs 1.6376 ms (-12.5 %), and 1.4310 vs "
                 "1.6334 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint; 786.1 M against 892.8 M VALU instructions per launch; "
                 "profiles/d_lean_headline_ab.txt")
KERNEL_LEAN_START = "_ZN7tinympc25k_admm_solve_d_lean_startILi12ELi4ELi50ELb1ELi4ELi25EEEvNS_11SolveParamsE"
SOURCE_LEAN_START = "tinympc_lstart_d.hip"
RECORD_LEAN_START = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_lean_start.json")
# what was measured for its recorded code (profiles/d_lean_start_headline_ab.txt)
LEAN_START_MEASURED = ("kernel 1.409 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_lean_start_kernel_stats.csv); tools/headline_ab.py, one box, against "
                       "the parent build's lean kernel (7,091 instructions, headline_kernel_code_d_lean.json) and the hoist-only build: 1.4350 / 1.4222 / 1.3987 ms "
                       "(-0.9 %, -2.5 %), and 1.4256 / 1.4181 / 1.3942 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint step by step; 764.5 M "
                       "against 786.1 M VALU instructions per launch; profiles/d_lean_start_headline_ab.txt")
KERNEL_LEAN_TRIM = "_ZN7tinympc24k_admm_solve_d_lean_trimILi12ELi4ELi50ELb1ELi4ELi25EEEvNS_11SolveParamsE"
SOURCE_LEAN_TRIM = "tinympc_ltrim_d.hip"
RECORD_LEAN_TRIM = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_lean_trim.json")
# what was measured for its recorded code (profiles/d_lean_trim_headline_ab.txt)
LEAN_TRIM_MEASURED = ("kernel 1.384 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_lean_trim_kernel_stats.csv); tools/headline_ab.py, one box, against "
                      "the parent build's lean-start kernel (7,152 instructions, headline_kernel_code_d_lean_start.json): 1.3822 vs 1.3991 ms (-1.2 %), and 1.3791 vs "
                      "1.3945 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint; 4.0 M against 43.9 M scalar and 763.7 M against 764.5 M VALU "
                      "instructions per launch; profiles/d_lean_trim_headline_ab.txt")
KERNEL_LEAN_SHARE = "_ZN7tinympc25k_admm_solve_d_lean_shareILi12ELi4ELi50ELb1ELi4ELi25EEEvNS_11SolveParamsE"
SOURCE_LEAN_SHARE = "tinympc_lshare_d.hip"
RECORD_LEAN_SHARE = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_lean_share.json")
# what was measured for its recorded code (profiles/d_lean_share_headline_ab.txt)
LEAN_SHARE_MEASURED = ("kernel 1.375 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_lean_share_kernel_stats.csv); tools/headline_ab.py, one box, against "
                       "the parent build's trimmed kernel (7,091 instructions, headline_kernel_code_d_lean_trim.json): 1.3689 vs 1.3844 ms (-1.1 %), and 1.3707 vs "
                       "1.3888 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint; 68.0 M against 87.5 M LDS and 763.7 M against 763.7 M VALU "
                       "instructions per launch; profiles/d_lean_share_headline_ab.txt")
KERNEL_LEAN_PARK = "_ZN7tinympc24k_admm_solve_d_lean_parkILi12ELi4ELi50ELb1ELi4ELi25EEEvNS_11SolveParamsE"
SOURCE_LEAN_PARK = "tinympc_lpark_d.hip"
RECORD_LEAN_PARK = os.path.join(ROOT, "tests", "golden", "headline_kernel_code_d_lean_park.json")
# what was measured for its recorded code (profiles/d_lean_park_headline_ab.txt)
LEAN_PARK_MEASURED = ("kernel 1.371 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_lean_park_kernel_stats.csv; the parent's 1.410 on the same box); tools/headline_ab.py, "
                      "one box, against the parent build's shared kernel (9,241 instructions, headline_kernel_code_d_lean_share.json): 1.3563 vs 1.3738 ms (-1.3 %), and 1.3559 vs "
                      "1.3742 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint; 48.5 M against 68.0 M LDS and 763.7 M against 763.7 M VALU "
                      "instructions per launch; profiles/d_lean_park_headline_ab.txt")


def compiler_version() -> str:
    try:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout
    except Exception:
        return "unknown"
    m = re.search(r"clang version [^\n]+", out)
    return m.group(0).strip() if m else out.strip().splitlines()[0]


def current_hash(kernel: str = KERNEL, source: str = "tinympc_solve_d.hip") -> dict | None:
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    path = ge.device_asm_path(source)
    if not os.path.exists(path):
        return None
    text = open(path).read()
    m = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    if not m:
        return None
    lines = []
    for line in m.group(1).split("\n"):
        t = line.split(";")[0].rstrip()
        if t.startswith(".LBB"):
            lines.append("L:")
        elif t.startswith("\t") and not t.strip().startswith("."):
            lines.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t.strip()))
    return {"kernel": kernel, "instructions": sum(1 for x in lines if x != "L:"), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(),
            "compiler": compiler_version()}


if __name__ == "__main__":
    h = current_hash()
    if h is None:
        sys.exit("no build assembly: run __graft_entry__.build() first")
    print(json.dumps(h, indent=1))
    lean = current_hash(KERNEL_LEAN, SOURCE_LEAN)
    if lean is not None:
        print(json.dumps(lean, indent=1))
    start = current_hash(KERNEL_LEAN_START, SOURCE_LEAN_START)
    if start is not None:
        print(json.dumps(start, indent=1))
    trim = current_hash(KERNEL_LEAN_TRIM, SOURCE_LEAN_TRIM)
    if trim is not None:
        print(json.dumps(trim, indent=1))
    share = current_hash(KERNEL_LEAN_SHARE, SOURCE_LEAN_SHARE)
    if share is not None:
        print(json.dumps(share, indent=1))
    park = current_hash(KERNEL_LEAN_PARK, SOURCE_LEAN_PARK)
    if park is not None:
        print(json.dumps(park, indent=1))
    if "--record" in sys.argv:
        h["measured"] = ("kernel 1.647 ms avg (8,192 x 200 iterations, bench.py on MI355X; profiles/d_fold_kernel_stats.csv); tools/headline_ab.py, one box, "
                         "against the build before knot 0 and the backward tail were folded (4,257 instructions): 1.6350 vs 1.6733 ms (-2.3 %), and "
                         "1.6391 vs 1.6752 ms at TINY_D_PAD=1, four interleaved rounds each, ranges disjoint; profiles/d_fold_headline_ab.txt")
        with open(RECORD, "w") as f:
            json.dump(h, f, indent=1)
            f.write("\n")
        print("recorded", RECORD)
    if "--record-lean" in sys.argv:
        if lean is None:
            sys.exit("no assembly of the lean kernel: run __graft_entry__.build() first")
        lean["measured"] = LEAN_MEASURED
        with open(RECORD_LEAN, "w") as f:
            json.dump(lean, f, indent=1)
            f.write("\n")
        print("recorded", RECORD_LEAN)
    if "--record-lean-start" in sys.argv:
        if start is None:
            sys.exit("no assembly of the lean kernel with LDS starts: run __graft_entry__.build() first")
        start["measured"] = LEAN_START_MEASURED
        with open(RECORD_LEAN_START, "w") as f:
            json.dump(start, f, indent=1)
            f.write("\n")
        print("recorded", RECORD_LEAN_START)
    if "--record-lean-trim" in sys.argv:
        if trim is None:
            sys.exit("no assembly of the trimmed lean kernel: run __graft_entry__.build() first")
        trim["measured"] = LEAN_TRIM_MEASURED
        with open(RECORD_LEAN_TRIM, "w") as f:
            json.dump(trim, f, indent=1)
            f.write("\n")
        print("recorded", RECORD_LEAN_TRIM)
    if "--record-lean-share" in sys.argv:
        if share is None:
            sys.exit("no assembly of the shared lean kernel: run __graft_entry__.build() first")
        share["measured"] = LEAN_SHARE_MEASURED
        with open(RECORD_LEAN_SHARE, "w") as f:
            json.dump(share, f, indent=1)
            f.write("\n")
        print("recorded", RECORD_LEAN_SHARE)
    if "--record-lean-park" in sys.argv:
        if park is None:
            sys.exit("no assembly of the lean kernel with the run's own slot split: run __graft_entry__.build() first")
        park["measured"] = LEAN_PARK_MEASURED
        with open(RECORD_LEAN_PARK, "w") as f:
            json.dump(park, f, indent=1)
            f.write("\n")
        print("recorded", RECORD_LEAN_PARK)
