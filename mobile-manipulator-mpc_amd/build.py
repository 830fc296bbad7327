"""Builds csrc/libmmpc.so for gfx950 with hipcc (cross-compiles without a GPU), and on demand the shape libraries
csrc/shapes/libmmpc_shape_<kind>_<N>_<M>.so: the specialised kernels of one (kind, N, M) each (csrc/mmpc_shape.hip)."""
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(CSRC, "libmmpc.so")
SHAPES = os.path.join(CSRC, "shapes")
SOURCES = ["mmpc_hip.hip"]
HEADERS = ["mmpc_core.h", "mmpc_tile.h", "mmpc_fast.h", "mmpc_fast_kernel.h", "mmpc_fast_iter.inc", "mmpc_fast_a1r.inc", "mmpc_fast_a1s.inc", "mmpc_fast_d2.inc", "mmpc_ik.h", "mmpc_tick.h", "mmpc_mission.h", "mmpc_manipulate.h", "mmpc_guess.h", "mmpc_round.h", "mmpc_suspend.h", os.path.join("..", "..", "include", "mmpc.h")]
SHAPE_SOURCE = "mmpc_shape.hip"


def _stale(out=LIB, extra=()):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS + list(extra))


def source_tag():
    """64 bits of a hash over the names and contents of the kernel sources (SOURCES + HEADERS).  libmmpc.so and every shape
    library are compiled with it (-DMMPC_SOURCE_TAG); mmpc_load_shape_library refuses a library with another one."""
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    return int.from_bytes(h.digest()[:8], "big")


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else "hipcc"


def _flags(tag):
    # -amdgpu-mfma-vgpr-form: the Riccati tiles stay in VGPRs (the pivots are read back by VALU instructions after every
    # rank-one MFMA; from AGPRs that is a v_accvgpr_read per word): +1.1 % on C4 and C5
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC", "-shared",
            "-DMMPC_SOURCE_TAG=0x%016xULL" % tag]


def extension_command():
    """the hipcc command line of libmmpc.so"""
    return [_hipcc()] + _flags(source_tag()) + ["-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES] + ["-ldl"]


def build_extension(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> csrc/libmmpc.so (in-tree, so that it travels with the repo)."""
    if not force and not _stale():
        return LIB
    cmd = extension_command()
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


def shape_library_path(kind, N, M):
    return os.path.join(SHAPES, "libmmpc_shape_%d_%d_%d.so" % (int(kind), int(N), int(M)))


def shape_library_current(kind, N, M):
    """the shape's library exists and is no older than the kernel sources (as build_extension judges libmmpc.so)"""
    return not _stale(shape_library_path(kind, N, M), (SHAPE_SOURCE,))


def shape_command(kind, N, M, out=None, tag=None):
    """the hipcc command line of a shape library: the flags and the source tag of libmmpc.so, and the shape"""
    out = out or shape_library_path(kind, N, M)
    return [_hipcc()] + _flags(source_tag() if tag is None else tag) + \
           ["-DMMPC_SHAPE_KIND=%d" % int(kind), "-DMMPC_SHAPE_N=%d" % int(N), "-DMMPC_SHAPE_M=%d" % int(M), "-o", out,
            os.path.join(CSRC, SHAPE_SOURCE)]


def shape_supported(kind, N, M):
    """mmpc_shape_supported: (kind, N, M) lies inside the envelope of the specialised template"""
    from . import _capi
    return bool(_capi.lib().mmpc_shape_supported(int(kind), int(N), int(M)))


def build_shape_library(kind, N, M, force=False, verbose=False, out=None, tag=None):
    """hipcc --offload-arch=gfx950 -> csrc/shapes/libmmpc_shape_<kind>_<N>_<M>.so: the six specialised kernels of the shape
    (one to two minutes; hipcc runs as a child process).  ValueError - before anything is compiled - for a shape outside
    the template's envelope (mmpc_shape_supported).  out, tag: another output file / source tag (tests)."""
    kind, N, M = int(kind), int(N), int(M)
    if not shape_supported(kind, N, M):
        raise ValueError("(kind, N, M) = (%d, %d, %d) is outside the envelope of the specialised kernels (mmpc_shape_supported)" % (kind, N, M))
    path = out or shape_library_path(kind, N, M)
    if not force and out is None and tag is None and shape_library_current(kind, N, M):
        return path
    return _compile_shape(kind, N, M, path, tag, verbose)


def _compile_shape(kind, N, M, path, tag=None, verbose=False):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp.%d" % os.getpid()      # (another process may be loading the file that is there)
    cmd = shape_command(kind, N, M, tmp, tag)
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.check_call(cmd, cwd=CSRC)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def build_many(shapes, force=False, jobs=16):
    """libmmpc.so (when stale) and the libraries of `shapes` (those that are stale), compiled side by side: at most `jobs`
    (never more than 16) hipcc processes at a time.  The shapes are checked against mmpc_shape_supported once the library is
    there; a shape outside the envelope does not compile (the template asserts the same predicate)."""
    from concurrent.futures import ThreadPoolExecutor
    shapes = [tuple(int(v) for v in s) for s in shapes]
    work = [lambda: build_extension(force=force)]
    for s in shapes:
        if force or not shape_library_current(*s):
            work.append(lambda s=s: _compile_shape(*s, shape_library_path(*s)))
    with ThreadPoolExecutor(max(1, min(int(jobs), 16))) as ex:
        for f in [ex.submit(w) for w in work]:
            f.result()
    for s in shapes:
        if not shape_supported(*s):
            raise ValueError("(kind, N, M) = %r is outside the envelope of the specialised kernels" % (s,))
    return [shape_library_path(*s) for s in shapes]


def load_shape_library(path):
    """mmpc_load_shape_library; RuntimeError with the library's text when it is refused"""
    from . import _capi
    L = _capi.lib()
    rc = L.mmpc_load_shape_library(os.fsencode(path))
    if rc != 0:
        raise RuntimeError("mmpc_load_shape_library failed (%d): %s" % (rc, (L.mmpc_last_error(None) or b"").decode()))
    return path
