"""hipcc build recipes (gfx950 only, in-tree outputs so the .so files travel with gpurun snapshots)."""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
QMM_SO = PKG / "libggml_mi355x_qmm.so"
PLUGIN_SO = PKG / "libggml-mi355x.so"
# a copy of the plugin kept with the other binaries built from the ggml tree (oracle/_ref, never in git): a checkout on a
# machine without that tree takes the module from there.  A directory of its own: next to the reference's executables it
# would sit where ggml looks for backend modules by name, and under the fingerprint of the sources it was compiled from (plugin_prebuilt):
# oracle/_ref outlives a checkout and may serve several commits, and a module of other sources must never stand in for this tree's
PLUGIN_PREBUILT_DIR = ROOT / "oracle" / "_ref" / "plugin"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GGML_SRC = Path(os.environ.get("GGML_SRC_DIR", "/root/reference/ggml"))


def _newer(target: Path, sources) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(Path(s).stat().st_mtime <= t for s in sources)


def build_qmm(force: bool = False) -> Path:
    """the kernel library behind include/ggml_mi355x_qmm.h and include/ggml_mi355x_ops.h: one object per translation unit
    (qmm_api.hip = the quantized MUL_MAT path with, as its section qmm_prefill.hiph, the prompt-batch launches, qmm_matvec.hip = the few-token mat-vec kernels, the one unit compiled with kernel-argument preload, qmm_ops.hip = the glue ops (what they launch: qmm_glue_plan.h) and, as its sections qmm_attn.hiph (with qmm_attn_rows.hiph), the attention launches, qmm_kcache.hiph, the Q8_0 K cache, qmm_kblk.hiph, a K cache in Q4_0 / Q4_1 / Q5_0 / Q5_1, and qmm_ropekq.hiph, the one-launch rope and store into such caches (planned by qmm_kcache_plan.h, qmm_kblk_plan.h and qmm_ropekq_plan.h), qmm_comm.hip = the RCCL exchange of a one-process row split), rebuilt only when its sources changed"""
    headers = sorted(CSRC.glob("qmm_*.hiph")) + sorted(CSRC.glob("qmm_*.h")) + sorted((ROOT / "include").glob("ggml_mi355x_*.h"))
    units = [CSRC / "qmm_api.hip", CSRC / "qmm_matvec.hip", CSRC / "qmm_ops.hip", CSRC / "qmm_comm.hip"]
    if not force and _newer(QMM_SO, units + headers):
        return QMM_SO
    if not shutil.which(HIPCC):
        # a library older than its sources is never used silently: a stale kernel must not be tested or benchmarked
        raise RuntimeError("hipcc not found and libggml_mi355x_qmm.so is " + ("older than its sources" if QMM_SO.exists() else "missing"))
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fno-slp-vectorize"]
    # the leading scalar parameters of the mat-vec kernels arrive in SGPRs (csrc/qmm_matvec.hip); the flag moves every kernel of a unit
    unit_flags = {"qmm_matvec.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=8"]}
    objs, jobs = [], []
    for u in units:
        obj = CSRC / (u.stem + ".o")
        objs.append(obj)
        if force or not _newer(obj, [u] + headers):
            jobs.append(subprocess.Popen([HIPCC, *flags, *unit_flags.get(u.name, []), "-c", str(u), "-o", str(obj)]))
    for j in jobs:
        if j.wait() != 0:
            raise subprocess.CalledProcessError(j.returncode, j.args)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(QMM_SO), *map(str, objs), "-ldl"], check=True)
    return QMM_SO


def have_ggml_headers() -> bool:
    return (GGML_SRC / "include" / "ggml-backend.h").exists() and (GGML_SRC / "src" / "ggml-backend-impl.h").exists()


def plugin_sources() -> list[Path]:
    """everything the plugin module is compiled from (one translation unit, ggml-mi355x.cpp, which includes the other sections)"""
    return [CSRC / "ggml-mi355x.cpp"] + sorted(CSRC.glob("mi355x_*")) + [CSRC / "qmm_switches.h", CSRC / "qmm_matvec_plan.h", CSRC / "qmm_types.h",
            ROOT / "include" / "ggml-mi355x.h", ROOT / "include" / "ggml_mi355x_qmm.h", ROOT / "include" / "ggml_mi355x_ops.h"]


def plugin_prebuilt() -> Path:
    """where the kept copy of the module built from THIS tree's plugin sources lives: a directory named by the hash of their contents"""
    h = hashlib.sha256()
    for f in plugin_sources():
        h.update(f.name.encode() + b"\0" + f.read_bytes() + b"\0")
    return PLUGIN_PREBUILT_DIR / h.hexdigest()[:16] / "libggml-mi355x.so"


def build_plugin(force: bool = False) -> Path | None:
    """the ggml backend plugin (GGML_BACKEND_DL module).  It is compiled against the ggml headers of the
    llama.cpp tree it will be loaded into (here: the reference tree, in place) and a copy is kept in
    oracle/_ref/plugin/<hash of the plugin sources>; when that tree is not present the module is taken from the copy made from
    the same sources (it finds the kernel library next to itself, rpath $ORIGIN), or the module already in place, if any, is kept.
    A copy made from other sources (another commit's) is never used."""
    src = CSRC / "ggml-mi355x.cpp"              # one translation unit: it includes the other sections (mi355x_*.cpp, one per concern)
    if not src.exists():
        return None
    srcs = plugin_sources()
    prebuilt = plugin_prebuilt()
    if not force and _newer(PLUGIN_SO, srcs + [QMM_SO]):
        return PLUGIN_SO
    if not have_ggml_headers() or not (shutil.which("g++") or shutil.which("c++")):
        # (whatever the dates say: a module left in place by a build of other sources may well be the younger file)
        if prebuilt.exists() and (not PLUGIN_SO.exists() or prebuilt.read_bytes() != PLUGIN_SO.read_bytes()):
            shutil.copy2(prebuilt, PLUGIN_SO)
        return PLUGIN_SO if PLUGIN_SO.exists() else None
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-DGGML_BACKEND_DL", "-DGGML_BACKEND_BUILD",
           "-DGGML_BACKEND_SHARED", "-DGGML_SHARED",
           f"-I{GGML_SRC / 'include'}", f"-I{GGML_SRC / 'src'}", f"-I{ROOT / 'include'}",
           str(src), "-o", str(PLUGIN_SO), f"-L{PKG}", "-lggml_mi355x_qmm", "-Wl,-rpath,$ORIGIN"]
    subprocess.run(cmd, check=True)
    prebuilt.parent.mkdir(parents=True, exist_ok=True)
    shutil.copy2(PLUGIN_SO, prebuilt)
    return PLUGIN_SO


def build_all(force: bool = False):
    return build_qmm(force), build_plugin(force)


if __name__ == "__main__":
    print(build_all(force=True))
