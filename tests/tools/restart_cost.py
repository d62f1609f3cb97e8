#!/usr/bin/env python3
"""GPU box: what a restart image costs (include/elmk.h "restart").  Tier A state tiled to each column count; per count it reports,
as the median of `rounds` repeats:
  - the image's bytes per column (no history entries);
  - elmk_restart_save into pageable host memory and into pinned host memory (hipHostMalloc), elmk_restart_load from pageable memory
    (two passes over the link: verify, then scatter);
  - the route a driver has without it: one elmk_download per field the image holds, in the SoA layout (no transpose) and in the
    reference's [column][level] layout (the device transposes through its staging buffer);
  - the link bound: one pinned hipMemcpy of the image's bytes from device memory, and the spec-sheet line (PCIe Gen5 x16, 63 GB/s).
Column counts that do not fit into the host's available memory (three images and the download route's arrays) are skipped.
python tests/tools/restart_cost.py [--cols 1000000,10000000] [--rounds 3] [--out profiles/r10_restart_cost.jsonl]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import _lib as L  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

PCIE_SPEC_GBS = 63.0


def hip_runtime():
    L.load()
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), None)
    hip = C.CDLL(path)
    P = C.c_void_p
    for name, args in (("hipMalloc", [C.POINTER(P), C.c_size_t]), ("hipFree", [P]), ("hipHostMalloc", [C.POINTER(P), C.c_size_t, C.c_uint]),
                       ("hipHostFree", [P]), ("hipMemcpy", [P, P, C.c_size_t, C.c_int]), ("hipDeviceSynchronize", [])):
        getattr(hip, name).argtypes = args
        getattr(hip, name).restype = C.c_int
    return hip


def mem_available():
    for ln in open("/proc/meminfo"):
        if ln.startswith("MemAvailable:"):
            return int(ln.split()[1]) * 1024
    return 0


def timed(fn, rounds):
    fn()
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def measure(cols, rounds, hip):
    D, _ = CL.bench.build_state(cols, 0, "A", 0x5EEDE1A0)
    nbytes = D.restart_size()
    names = [k for k in D.fields if st.field_class(k) in (st.CLASS_PROGNOSTIC, st.CLASS_SURFACE)]
    field_bytes = sum(cols * D.fields[k][1] * np.dtype(D.fields[k][2]).itemsize for k in names)
    img = np.empty(nbytes, np.uint8)
    img[:] = 0
    pinned = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(pinned), nbytes, 0) == 0
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), nbytes) == 0
    outs = {k: np.empty((D.fields[k][1], cols) if D.fields[k][1] > 1 else (cols,), D.fields[k][2]) for k in names}
    outs_cm = {k: np.empty((cols, D.fields[k][1]) if D.fields[k][1] > 1 else (cols,), D.fields[k][2]) for k in names}
    try:
        save = timed(lambda: D.lib.elmk_restart_save(D.ctx, 0, img.ctypes.data, nbytes), rounds)
        save_pinned = timed(lambda: D.lib.elmk_restart_save(D.ctx, 0, pinned, nbytes), rounds)
        load = timed(lambda: D.restart_load(img), rounds)
        per_field = timed(lambda: [D.download(k, layout=st.LAYOUT_SOA, out=outs[k]) for k in names], rounds)
        per_field_cm = timed(lambda: [D.download(k, out=outs_cm[k]) for k in names], rounds)
        link = timed(lambda: (hip.hipMemcpy(pinned, dev, nbytes, 2), hip.hipDeviceSynchronize()), rounds)
    finally:
        hip.hipHostFree(pinned)
        hip.hipFree(dev)
        D.close()
    gbs = lambda ms: nbytes / (ms * 1e-3) / 1e9  # noqa: E731
    return dict(tool="restart_cost", cols=cols, lib=os.path.basename(L.LIB_PATH), image_bytes=nbytes, bytes_per_column=nbytes / cols,
                fields=len(names), field_bytes=field_bytes, save_ms=save, save_pinned_ms=save_pinned, load_ms=load,
                per_field_download_ms=per_field, per_field_download_colmajor_ms=per_field_cm, pinned_copy_ms=link, save_gbs=gbs(save), save_pinned_gbs=gbs(save_pinned),
                load_gbs=gbs(load), pinned_copy_gbs=gbs(link), save_vs_per_field=per_field / save, save_vs_per_field_colmajor=per_field_cm / save,
                save_fraction_of_pinned_copy=link / save, save_pinned_fraction_of_pinned_copy=link / save_pinned,
                pinned_copy_fraction_of_spec=gbs(link) / PCIE_SPEC_GBS, rounds=rounds)


def main():
    a = CL.cli("1000000,10000000", 3, out=True)
    hip = hip_runtime()

    def one(cols):
        probe = st.ELMState(64)
        per_col = probe.restart_size() / 64
        probe.close()
        need = 3.2 * per_col * cols
        if need > 0.8 * mem_available():
            return dict(tool="restart_cost", cols=cols, skipped=f"needs ~{need / 2**30:.1f} GiB of host memory, "
                                                                f"{mem_available() / 2**30:.1f} GiB available")
        return measure(cols, a.rounds, hip)

    CL.emit_each(a, one)


if __name__ == "__main__":
    main()
