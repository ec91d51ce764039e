"""Builds the HIP libraries for gfx950 with hipcc, in-tree.

  libczk_hip.so      the PRODUCT: the kernels a prover runs + the C ABI of include/czk.h.  Reads no environment variables; tuning goes
                     through czk_ctx_set_option.
  libczk_hip_lab.so  the LAB build (-DCZK_LAB): the same sources plus the measured-and-rejected variants kept for A/B runs (csrc/lab/:
                     batched-affine rounds, safegcd inversion, interleaved multiply-add chains, Karatsuba Fq2; the lane-pair G2 accumulate
                     kernel, the saturated accumulate / reduction kernels) and the CZK_* environment switches of the measurement tools,
                     which it translates into options.  Every ABI symbol, plus the probe: csrc/lab/arith_probe.hip (LAB_SOURCES) exports
                     czk_lab_arith_probe, which runs one function on raw limbs: of the unsaturated arithmetic headers for
                     tests/test_lazy_arith.py, and of the saturated field.h / tower.h / curve.h (csrc/lab/sat_probe.h) for
                     tests/test_sat_arith.py.  The saturated probes are compiled in both forms field.h is built in: with the Montgomery
                     multiply inlined in arith_probe.hip, and with -DCZK_NOINLINE_MUL (the form of pairing.hip, the only one the Fq6 / Fq12
                     tower has) in csrc/lab/sat_probe.hip.  csrc/lab/msm_sort_probe.hip exports czk_lab_msm_sort, which runs the digit sort of
                     one MSM call (msm_sort.hip) on its own and returns its arrays and dimensions for tests/test_msm_digits.py; csrc/lab/msm_bucket_probe.hip exports
                     czk_lab_msm_buckets, which runs the bucket accumulation and reduction (msm.hip's stage bodies) on entry lists the caller wrote and
                     returns every bucket, the rare-path counters and the lane results for tests/test_msm_buckets.py.  csrc/lab/merkle_probe.hip exports
                     czk_lab_merkle_commit, the tree of czk_fr_merkle_commit in the form that was not shipped (one workgroup per subtree), for tools/fri_bench.py
                     and tests/test_merkle_fri.py.  csrc/lab/ntt_pass_probe.hip exports czk_lab_ntt_pass, which launches ONE pass of the second-generation NTT
                     (ntt_pass.hip: launch_ntt2_pass or the fused launch_ntt2_final_first) on a buffer the caller wrote, at any legal (log_d, s_lo, K), and returns
                     the whole output buffer with its sentinel-filled guard tail for tests/test_ntt_pass.py.  Loaded by tests through Context(lab=True) and by tools through CZK_LIB_PATH;
                     never by the provers.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container as well as on the GPU box.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libczk_hip.so")
LIB_LAB = os.path.join(HERE, "libczk_hip_lab.so")
# (source, extra flags).  msm.hip (the pipeline), msm_sort.hip (the digit sort) and msm_bases.hip (keys, window tables, setup kernels) are built with the Montgomery
# multiply out of line (see field.h CZK_NOINLINE_MUL); the hot kernels keep it inlined.  core.hip is host code only (the host-side
# group operations): out of line too, 14 s instead of 4.5 min of host compilation.
SOURCES = [("core.hip", ["-DCZK_NOINLINE_MUL"]), ("lanes.hip", ["-DCZK_NOINLINE_MUL"]), ("ntt.hip", []), ("ntt_pass.hip", []), ("ntt_mixed.hip", []), ("fr_vec.hip", []), ("witness_map.hip", []), ("msm.hip", ["-DCZK_NOINLINE_MUL"]), ("msm_sort.hip", ["-DCZK_NOINLINE_MUL"]),
           ("msm_bases.hip", ["-DCZK_NOINLINE_MUL"]), ("msm_acc_g1.hip", []),
           ("msm_acc_g2.hip", []), ("msm_red_g2.hip", []), ("msm_heavy_g2.hip", []), ("poly.hip", []), ("share.hip", []), ("share_mul.hip", []), ("gsz_mul.hip", []), ("gsz_dn.hip", []), ("net.hip", ["-DCZK_NOINLINE_MUL"]), ("net_rounds.hip", ["-DCZK_NOINLINE_MUL"]),
           ("pairing.hip", ["-DCZK_NOINLINE_MUL"]), ("fixed_base.hip", []), ("point_codec.hip", ["-DCZK_NOINLINE_MUL"]),
           ("point_ops.hip", ["-DCZK_NOINLINE_MUL"]), ("group_share.hip", ["-DCZK_NOINLINE_MUL"]), ("pairing_share.hip", ["-DCZK_NOINLINE_MUL"]), ("kzg.hip", ["-DCZK_NOINLINE_MUL"]), ("marlin_index.hip", []), ("plonk_layout.hip", []), ("commit_tree.hip", []), ("merkle.hip", []), ("fs.hip", ["-DCZK_NOINLINE_MUL"])]
# lab library only: never compiled into, nor linked with, the product library
LAB_SOURCES = [(os.path.join("lab", "arith_probe.hip"), []), (os.path.join("lab", "sat_probe.hip"), ["-DCZK_NOINLINE_MUL"]),
               (os.path.join("lab", "msm_sort_probe.hip"), ["-DCZK_NOINLINE_MUL"]), (os.path.join("lab", "msm_bucket_probe.hip"), ["-DCZK_NOINLINE_MUL"]),
               (os.path.join("lab", "merkle_probe.hip"), []), (os.path.join("lab", "ntt_pass_probe.hip"), [])]
HEADERS = ["field.h", "curve.h", "czk_internal.h", "call.h", "net.h", "sha256.h", "sha256_dev.h", "blake2s.h", "chacha20.h", "merkle_hash.h", "merkle_tree_plain.h", "pow_tables.h", "msm_acc.h", "fq2p.h", "fq2pu.h", "fqu.h", "fru.h", "fru_constants.inc", "ntt_pass.h", "te.h", "te_constants.inc", "tower.h", "pairing_steps.h", "pairing_constants.inc",
           os.path.join("..", "..", "include", "czk.h")]
LAB_HEADERS = [os.path.join("lab", h) for h in ("msm_aff.h", "fq_safegcd.h", "fqu_il.h", "fqu_mad_il.inc", "fq2u_karatsuba.h", "arith_probe.h", "sat_probe.h", "merkle_tree_fused.h", "ntt_pass_probe.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result", "-Wno-pass-failed", "-I" + CSRC]
# parallel hipcc jobs: CZK_BUILD_JOBS, else the MAX_JOBS a build host sets (a container's os.cpu_count() is the whole machine's), else all cores
MAX_JOBS = int(os.environ.get("CZK_BUILD_JOBS", "0")) or int(os.environ.get("MAX_JOBS", "0")) or max(4, (os.cpu_count() or 8))


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _plan(lab: bool, force: bool):
    hdrs = [os.path.join(CSRC, h) for h in HEADERS + (LAB_HEADERS if lab else [])]
    objdir = os.path.join(CSRC, "obj_lab" if lab else "obj")
    os.makedirs(objdir, exist_ok=True)
    objs, jobs = [], []
    for src, extra in SOURCES + (LAB_SOURCES if lab else []):
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, os.path.basename(src).replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([HIPCC] + FLAGS + extra + (["-DCZK_LAB"] if lab else []) + ["-c", s, "-o", o])
    return objs, jobs


def build(force: bool = False, verbose: bool = False, lab: bool = True) -> str:
    """Builds the product library, and the lab library too unless lab=False.  Returns the product library's path."""
    import time

    def run(cmd):
        t0 = time.time()
        subprocess.check_call(cmd)
        if verbose:
            print("%6.1fs  %s" % (time.time() - t0, " ".join(cmd[-4:])), file=sys.stderr)

    targets = [(LIB, False)] + ([(LIB_LAB, True)] if lab else [])
    plans = [(lib, *_plan(is_lab, force)) for lib, is_lab in targets]
    jobs = [j for _, _, js in plans for j in js]
    if jobs:
        with ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(jobs))) as ex:
            list(ex.map(run, jobs))
    for lib, objs, js in plans:
        if js or _stale(lib, objs):
            run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, lab="--no-lab" not in sys.argv))
