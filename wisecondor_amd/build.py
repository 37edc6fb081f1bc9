"""Build libwisecondor_hip.so (gfx950) in-tree with hipcc.

`python -m wisecondor_amd.build` or `__graft_entry__.build()`.  The library is
plain HIP + a C ABI (include/wisecondor_hip.h); it links against nothing but
the HIP runtime, so it can be bound from ctypes, cgo, JNI, ...
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libwisecondor_hip.so")
SOURCES = ["ctx.hip", "newref.hip", "testpath.hip", "prep.hip", "eigh.hip", "convert.hip", "bamgpu.hip", "deflate.hip", "plot.hip", "pdf.hip", "export.hip", "tracks.hip", "spike.hip", "draw.hip", "crossval.hip", "robust.hip", "npzio.cpp", "bamio.cpp",
           "bamfile.cpp"]   # npzio.cpp, bamio.cpp, bamfile.cpp: host only (zip / pickle / zlib; BGZF / BAM)
# -fno-slp-vectorize: the SLP vectoriser pairs float32 operations into v_pk_add_f32 /
# v_pk_fma_f32; an in-place pair whose low half reads the destination's high half
# (v_pk_add_f32 v[74:75], v[84:85], v[74:75] op_sel:[0,1]) returned run-to-run different
# results on gfx950 in the threshold kernel.  Nothing here gains from packed float32 math.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found; set HIPCC")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "wisecondor_hip.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=True):
    """Compile every .hip source for gfx950 and link the shared library."""
    if not force and not needs_build():
        return LIB
    hipcc = _hipcc()
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        cmd = [hipcc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd)))
        objs.append(obj)
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s" % src)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB)
