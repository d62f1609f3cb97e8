"""What the tests share that is neither physics nor one feature's: the two array comparisons, the HIP runtime with a guarded stream
capture, and the example programs (build, run, the state.bin they read).  The context builder is helpers.device_state.  Each exists
once; a new feature's test starts from here (and from run_cases / hydrology_cases), not from a copy of another test file.  Asserts
here carry a message: the module is not rewritten by pytest."""
import contextlib
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def bits(a):
    """the bytes as stored"""
    return np.ascontiguousarray(a).tobytes()


def bits_f64(a):
    """the bytes of the values as fp64"""
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def words_f64(a):
    """the values as fp64, as an array of their 64-bit words"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """exact: the same shape, dtype and bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_nan(a, b):
    """bit for bit as fp64, a NaN matching any NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- the HIP runtime: streams, capture, replay ---------------------------------------------------------------------------------------
_HIP = None


def hip_runtime():
    """The HIP runtime this process already uses (loaded by libelmk): the same instance, so streams and graphs are shared."""
    global _HIP
    if _HIP is None:
        L.load()
        path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), None)
        assert path, "libamdhip64 is not loaded"
        hip = C.CDLL(path)
        P = C.c_void_p
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(P), C.c_uint]), ("hipStreamBeginCapture", [P, C.c_int]),
                           ("hipStreamEndCapture", [P, C.POINTER(P)]), ("hipGraphInstantiate", [C.POINTER(P), P, P, P, C.c_size_t]),
                           ("hipGraphLaunch", [P, P]), ("hipStreamSynchronize", [P]), ("hipGraphExecDestroy", [P]),
                           ("hipGraphDestroy", [P]), ("hipStreamDestroy", [P])):
            getattr(hip, name).argtypes = args
            getattr(hip, name).restype = C.c_int
        _HIP = hip
    return _HIP


class Capture:
    """What `captured` yields: the stream, and the graph once the capture has ended."""

    def __init__(self, hip):
        self.hip, self.stream, self.graph, self.capturing = hip, C.c_void_p(), C.c_void_p(), False

    def end(self):
        """End the capture now (`captured` does it on exit otherwise): calls after it run on the stream."""
        self.capturing = False
        rc = self.hip.hipStreamEndCapture(self.stream, C.byref(self.graph))
        assert rc == 0, f"hipStreamEndCapture returned {rc}"

    def replay(self, k):
        """Instantiate the captured graph, launch it k times on the stream, synchronise, destroy the executable graph."""
        hip, exe = self.hip, C.c_void_p()
        rc = hip.hipGraphInstantiate(C.byref(exe), self.graph, None, None, 0)
        assert rc == 0, f"hipGraphInstantiate returned {rc}"
        try:
            for i in range(k):
                rc = hip.hipGraphLaunch(exe, self.stream)
                assert rc == 0, f"hipGraphLaunch {i} returned {rc}"
            rc = hip.hipStreamSynchronize(self.stream)
            assert rc == 0, f"hipStreamSynchronize returned {rc}"
        finally:
            hip.hipGraphExecDestroy(exe)


@contextlib.contextmanager
def captured(*contexts):
    """A new non-blocking stream, made the stream of every context given and put into capture (thread-local mode) around the body.
    However the body ends, the capture is ended (unless cap.end() did), the graph destroyed, the contexts given their own streams
    back and the stream destroyed: a failing assert in the body leaves the contexts usable.  To replay, end the capture inside the
    body (cap.end()) and call cap.replay(k): the contexts are still on the stream then."""
    hip = hip_runtime()
    cap = Capture(hip)
    rc = hip.hipStreamCreateWithFlags(C.byref(cap.stream), 1)  # hipStreamNonBlocking
    assert rc == 0, f"hipStreamCreateWithFlags returned {rc}"
    try:
        for D in contexts:
            D.set_stream(cap.stream.value)
        rc = hip.hipStreamBeginCapture(cap.stream, 1)  # hipStreamCaptureModeThreadLocal
        assert rc == 0, f"hipStreamBeginCapture returned {rc}"
        cap.capturing = True
        try:
            yield cap
        except BaseException:
            if cap.capturing:  # the body's error is the one to report, not a status of the clean-up
                hip.hipStreamEndCapture(cap.stream, C.byref(cap.graph))
                cap.capturing = False
            raise
        if cap.capturing:
            cap.end()
    finally:
        if cap.graph.value:
            hip.hipGraphDestroy(cap.graph)
        for D in contexts:
            D.set_stream(None)
        hip.hipStreamDestroy(cap.stream)


# ---- the examples -------------------------------------------------------------------------------------------------------------------
def build_demo(name, tmp_path):
    """examples/<name>.cc compiled against include/ and libelmk into the directory tmp_path; returns the executable's path."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    libdir = os.path.dirname(L.LIB_PATH)
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".cc"), "-L" + libdir, "-lelmk", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def run_demo(exe, *args, timeout=600):
    """Run an example to its end; its exit status must be 0.  Returns the completed process (stdout, stderr as text)."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{os.path.basename(exe)} exited with {r.returncode}:\n{r.stdout}{r.stderr}"
    return r


def state_blob(S, dt, extra=()):
    """The state.bin the examples read (examples/demo_io.h), as bytes: the column count; every field of the oracle state S but
    err_flags (kind 0); the land unit, the scalars with dt, the parameter tables, the SNICAR tables and the snow-age tables (kind 1);
    then the records of `extra`, [(name, array)], kind 1.  A record: the name padded to 32 bytes, kind (int32), byte count (int64),
    the bytes."""
    n = next(iter(S.fields.values())).shape[0]
    blob = [struct.pack("<q", n)]

    def put(name, kind, arr):
        a = np.ascontiguousarray(arr)
        blob.append(name.encode().ljust(32, b"\0") + struct.pack("<iq", kind, a.nbytes) + a.tobytes())

    for k, v in S.fields.items():
        if k != "err_flags":
            put(k, 0, v)
    sc = S.scalars
    put("land", 1, np.array([sc["ltype"], sc["ctype"], sc["vtype"], sc["urbpoi"], sc["lakpoi"]], np.int32))
    put("scalars", 1, np.array([sc["dewmx"], sc["oldfflag"], sc["dayl"], sc["max_dayl"], dt], np.float64))
    for k in ("pft_psn", "pft_alb", "z0mr", "displar", "albsat", "albdry"):
        put(k, 1, getattr(S, k))
    for i, name in enumerate(L.SNICAR_NAMES):
        put(f"snicar/{i}", 1, S.snicar[name])
    put("age_tau", 1, S.snowage[0])
    put("age_kappa", 1, S.snowage[1])
    put("age_drdt0", 1, S.snowage[2])
    for name, arr in extra:
        put(name, 1, arr)
    return b"".join(blob)
