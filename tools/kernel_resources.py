"""Device assembly of every MPC translation unit at two source trees, per kernel symbol: whether the instructions are
byte-equal, and VGPRs / SGPRs / scratch / LDS / occupancy from -Rpass-analysis=kernel-resource-usage.

  python tools/kernel_resources.py PARENT_TREE THIS_TREE OUT.json [--work DIR]

Each unit is compiled with the Makefile's flags for its object plus -S --cuda-device-only and a fixed -cuid (so that
symbol names do not depend on the path); comments, directives and local labels' numbering are not compared: a kernel's
text is its instruction lines.  CPU only (hipcc cross-compiles)."""
import concurrent.futures as cf
import hashlib
import json
import os
import re
import subprocess
import sys

BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm",
        "-pragma-unroll-threshold=100000"]
NOLICM = ["-mllvm", "-disable-machine-licm"]
UNITS = {
    "mpc_inst_16": ("mpc_inst.hip", NOLICM + ["-DTGMPC_DPP_BC=1", "-DTGMPC_NN=16"]),
    "mpc_inst_32": ("mpc_inst.hip", NOLICM + ["-DTGMPC_DPP_BC=1", "-DTGMPC_NN=32"]),
    "mpc_inst_40": ("mpc_inst.hip", NOLICM + ["-DTGMPC_DPP_BC=1", "-DTGMPC_NN=40"]),
    "mpc_inst_80": ("mpc_inst.hip", NOLICM + ["-DTGMPC_DPP_BC=1", "-DTGMPC_NN=80", "-mllvm",
                                              "-amdgpu-sched-strategy=max-ilp"]),
    "mpc_inst_w3_40": ("mpc_inst_w3.hip", NOLICM + ["-mllvm", "-amdgpu-use-amdgpu-trackers=1", "-DTGMPC_NN=40"]),
    "split_inst": ("split_inst.hip", NOLICM),
    "trajmpc": ("trajmpc.hip", []),
}
COLS = {"vgpr": r"\bVGPRs: (\d+)", "sgpr": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
        "lds": r"LDS Size \[bytes/block\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)"}


def compile_unit(tree, unit, work):
    src, extra = UNITS[unit]
    out = os.path.join(work, unit + ".s")
    os.makedirs(work, exist_ok=True)
    cmd = (["/opt/rocm/bin/hipcc"] + BASE + extra + ["-S", "--cuda-device-only", "-cuid=0",
           "-Rpass-analysis=kernel-resource-usage", "-o", out, src])
    p = subprocess.run(cmd, cwd=os.path.join(tree, "trajectory_generation_amd", "csrc"), capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError(p.stderr[-2000:])
    return unit, out, p.stderr


def kernels(asm, remarks):
    """symbol -> (sha of the instruction lines, resource columns)"""
    res = {}
    for blk in remarks.split("Function Name: ")[1:]:
        sym = blk.split()[0]
        res[sym] = {k: int(re.search(rx, blk).group(1)) for k, rx in COLS.items() if re.search(rx, blk)}
    s = open(asm).read()
    out = {}
    for sym, cols in res.items():
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(sym), s, flags=re.M | re.S)
        if not m:
            continue
        ins = [ln.split(";")[0].strip() for ln in m.group(1).split("\n")]
        ins = [ln for ln in ins if ln and not ln.startswith((".", ";", "//"))]
        out[sym] = (hashlib.sha256("\n".join(ins).encode()).hexdigest()[:12], cols)
    return out


def main():
    parent, this, dst = sys.argv[1:4]
    work = sys.argv[sys.argv.index("--work") + 1] if "--work" in sys.argv else "/tmp/kernel_resources"
    jobs = [(t, u, os.path.join(work, n)) for n, t in (("parent", parent), ("final", this)) for u in UNITS]
    got = {"parent": {}, "final": {}}
    with cf.ThreadPoolExecutor(8) as ex:
        for (tree, _, w), (unit, out, err) in zip(jobs, ex.map(lambda j: compile_unit(*j), jobs)):
            got[os.path.basename(w)][unit] = kernels(out, err)
    table = []
    for unit in UNITS:
        for sym in sorted(got["final"][unit]):
            f = got["final"][unit][sym]
            p = got["parent"][unit].get(sym)
            table.append({"unit": unit, "symbol": sym, "parent_sha256": p and p[0], "final_sha256": f[0],
                          "byte_equal": bool(p) and p[0] == f[0], "parent": p and p[1], "final": f[1]})
    rec = {"kernels": len(table), "byte_equal": sum(r["byte_equal"] for r in table),
           "changed": [r for r in table if not r["byte_equal"]],
           "unchanged": [{"unit": r["unit"], "symbol": r["symbol"], "sha256": r["final_sha256"], **r["final"]}
                         for r in table if r["byte_equal"]]}
    json.dump(rec, open(dst, "w"), indent=1)
    print(json.dumps({k: rec[k] for k in ("kernels", "byte_equal")}), [r["symbol"] for r in rec["changed"]])


if __name__ == "__main__":
    main()
