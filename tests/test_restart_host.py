"""Restart images on the host: the field classes of include/elmk_restart.def (read through the ABI) checked with the oracle over the
whole per-step sequence, the numpy codec of the image format (elmkernels_amd/restart.py), and the new declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.support import ROOT

DT = 1800.0
SERIES = st.SERIES_FORCING + st.SERIES_PHENOLOGY
PRIMARY_VARS = ("snl", "snow_depth", "frac_sno", "int_snow", "snw_rds", "h2osoi_liq", "h2osoi_ice", "h2osoi_vol", "h2ocan", "h2osno",
                "h2osfc", "t_soisno", "t_grnd", "t_h2osfc", "t_h2osfc_bef", "nrad", "dz", "zsoi", "zisoi")
NEW_SYMBOLS = ("elmk_field_class", "elmk_restart_size", "elmk_restart_save", "elmk_restart_load")


def _classes():
    lib = L.load()
    return {lib.elmk_field_name(i).decode(): lib.elmk_field_class(i) for i in range(lib.elmk_num_fields())}


def test_every_field_has_one_class():
    lib = L.load()
    cls = _classes()
    assert len(cls) == lib.elmk_num_fields()
    assert set(cls.values()) <= {st.CLASS_PROGNOSTIC, st.CLASS_SURFACE, st.CLASS_FORCING, st.CLASS_DIAGNOSTIC}
    assert lib.elmk_field_class(-1) < 0 and lib.elmk_field_class(lib.elmk_num_fields()) < 0
    names = re.findall(r"^ELMK_RESTART_CLASS\((\w+),", open(os.path.join(ROOT, "include", "elmk_restart.def")).read(), re.M)
    assert sorted(names) == sorted(cls) and len(names) == len(set(names))


def test_forcing_is_exactly_the_series_fields():
    assert {k for k, c in _classes().items() if c == st.CLASS_FORCING} == set(SERIES)


def test_primary_vars_and_err_flags_are_saved():
    cls = _classes()
    for k in PRIMARY_VARS:
        assert cls[k] in (st.CLASS_PROGNOSTIC, st.CLASS_SURFACE), k
    assert cls["err_flags"] == st.CLASS_PROGNOSTIC


def _oracle_run(n, seed, tier):
    cols, scal, soil = synth.make_state(H.field_table_from_oracle(), n, tier=tier, seed=seed)
    S = H.oracle_state(cols, scal, soil)
    rng = np.random.default_rng(seed + 7)
    nrec = 16
    rec = {}
    for k in SERIES:
        a, b = cols[k][:, 0], cols[k][:, 1]
        t = np.linspace(0.0, 1.0, nrec)[:, None]
        rec[k] = np.abs((1 - t) * a[None] + t * b[None] + 0.01 * np.abs(a)[None] * rng.standard_normal((nrec, n)))
    rec["atm_prec"] = np.where(rng.random((nrec, n)) < 0.3, 0.0, rec["atm_prec"])
    return S, rec


def _step(S, rec, s):
    """The per-step sequence of elmk_run on the oracle, the series records supplied as the driver does."""
    for k in SERIES:
        S[k][...] = np.stack([rec[k][s], rec[k][s + 1]], axis=1)
    w2 = np.clip(0.25 + 0.5 * (s % 2) + 0.03 * np.arange(8) - 0.1, 0.0, 1.0)
    S.phenology(0.3 + 0.01 * s, 0.7 - 0.01 * s)
    S.get_forcing(1.0 - w2, w2)
    S.init_timestep()
    S.timestep7(DT)
    S.soil_temperature(DT)
    S.snow_hydrology(DT)
    S.surface_fluxes(DT)
    S.evaluate_conservation(DT)


def _poison(S, names, kind):
    for k in names:
        a = S[k]
        if a.dtype == np.float64:
            a[...] = np.nan if kind == 0 else 1e30
        else:
            a[...] = {np.dtype(np.int32): 987654, np.dtype(np.uint8): 0x5C, np.dtype(np.uint32): 0xDEADBEEF}[a.dtype]


@pytest.mark.parametrize("n,seed,tier,K,M", [(1024, 11, "B", 3, 4), (1024, 13, "W", 5, 5)])
@pytest.mark.parametrize("kind", [0, 1], ids=["nan", "large"])
def test_poisoned_non_image_fields_change_no_bit(n, seed, tier, K, M, kind):
    """After K chained steps every DIAGNOSTIC and FORCING field is poisoned at once; M more steps (with the forcing re-supplied)
    give every field the bits of the clean clone, and leave SURFACE and FORCING fields untouched."""
    cls = _classes()
    S, rec = _oracle_run(n, seed, tier)
    for s in range(K):
        _step(S, rec, s)
    clean, poisoned = S.clone(), S.clone()
    before = {k: S[k].copy() for k in S.fields}
    _poison(poisoned, [k for k, c in cls.items() if c in (st.CLASS_DIAGNOSTIC, st.CLASS_FORCING)], kind)
    for s in range(K, K + M):
        _step(clean, rec, s)
        _step(poisoned, rec, s)
    for k in S.fields:
        assert clean[k].tobytes() == poisoned[k].tobytes(), k
        if cls[k] == st.CLASS_SURFACE:
            assert clean[k].tobytes() == before[k].tobytes(), k
    # the forcing fields hold what the driver supplied last, nothing the step wrote
    for k in SERIES:
        assert clean[k].tobytes() == np.stack([rec[k][K + M - 1], rec[k][K + M]], axis=1).tobytes(), k


# ---- the codec ------------------------------------------------------------------------------------------------------------------
def test_fmix64_and_checksum_known_vectors():
    assert int(R.fmix64(0)) == 0
    assert int(R.fmix64(1)) == 0xB456BCFC34C2CB2C
    assert int(R.fmix64(0xFFFFFFFFFFFFFFFF)) == 0x64B5720B4B825F21
    # one element: fmix64(bits ^ fmix64(g * 64 + lev + 1))
    assert R.checksum(np.array([[1.0]]), 0) == int(R.fmix64(np.uint64(0x3FF0000000000000) ^ R.fmix64(1)))
    assert R.checksum(np.array([[7]], np.int32), 3) == int(R.fmix64(np.uint64(7) ^ R.fmix64(3 * 64 + 1)))
    # -1 as int32 is zero-extended
    assert R.checksum(np.array([[-1]], np.int32), 0) == int(R.fmix64(np.uint64(0xFFFFFFFF) ^ R.fmix64(1)))
    # position matters: the same values at other columns or levels sum differently
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert R.checksum(a, 0) != R.checksum(a, 1) and R.checksum(a, 0) != R.checksum(a[::-1].copy(), 0)
    assert R.checksum(a, 0) == 0xA37B91B642F84399


def _image(gcol0=0, n=37, gridded=False, seed=3):
    rng = np.random.default_rng(seed)
    h = np.zeros((), R.HEADER)
    h["magic"], h["version"], h["real_bytes"], h["schema_hash"] = R.MAGIC, R.VERSION, 8, 0x1234
    h["gcol0"], h["ncols"], h["tape_count"] = gcol0, n, [5, 2, 0, 0]
    ent = np.zeros(2, R.ENTRY)
    ent[0] = (0, 52, 0, 0, 0)
    ent[1] = (1, 52, 2, 1 if gridded else 0, 9 if gridded else 0)
    secs = [(R.FIELD, 29, 1, 1), (R.FIELD, 51, 20, 0), (R.FIELD, 167, 1, 2), (R.HISTORY, 0, 1, 0)]
    secs.append((R.GRIDDED, 1, 1, 0) if gridded else (R.HISTORY, 1, 1, 0))
    sec = np.zeros(len(secs), R.SECTION)
    data = []
    for i, (kind, fid, nlev, dt) in enumerate(secs):
        ext = 9 if kind == R.GRIDDED else n
        d = (rng.integers(0, 6, (nlev, ext)) if dt != 0 else rng.standard_normal((nlev, ext))).astype(R.ELEM[dt])
        sec[i] = (kind, fid, nlev, dt, ext, 0, R.checksum(d, 0 if kind == R.GRIDDED else gcol0))
        data.append(d)
    return R.build(h, ent, sec, data)


def test_merge_of_slices_is_the_image():
    img = _image(gcol0=100, n=37)
    R.verify(img)
    parts = [R.slice(img, 100, 10), R.slice(img, 110, 1), R.slice(img, 111, 26)]
    for p in parts:
        R.verify(p)
    assert R.merge(parts[::-1]).tobytes() == img.tobytes()


def test_checksums_add_over_column_ranges():
    img = _image(gcol0=0, n=37)
    a, b = R.slice(img, 0, 20), R.slice(img, 20, 17)
    for s, sa, sb in zip(R.parse(img)["sections"], R.parse(a)["sections"], R.parse(b)["sections"]):
        assert int(s["checksum"]) == (int(sa["checksum"]) + int(sb["checksum"])) % (1 << 64)


def test_damaged_images_are_refused(tmp_path):
    img = _image()
    p = R.parse(img)
    flipped = img.copy()
    flipped[int(p["sections"][1]["offset"]) + 5] ^= 1
    with pytest.raises(R.RestartError):
        R.verify(flipped)
    hdr = img.copy()
    hdr[20] ^= 1
    with pytest.raises(R.RestartError):
        R.verify(hdr)
    with pytest.raises(R.RestartError):
        R.verify(img[:-256])
    with pytest.raises(R.RestartError):
        R.verify(img[:50])
    R.write(tmp_path / "r.img", img)
    assert R.read(tmp_path / "r.img").tobytes() == img.tobytes()
    R.write(tmp_path / "t.img", img[:-8])
    with pytest.raises(R.RestartError):
        R.read(tmp_path / "t.img")


def test_gridded_images_do_not_merge_or_slice():
    img = _image(gridded=True)
    R.verify(img)
    with pytest.raises(R.RestartError):
        R.merge([img])
    with pytest.raises(R.RestartError):
        R.slice(img, 0, 5)
    with pytest.raises(R.RestartError):
        R.merge([_image(0, 10), _image(11, 10)])  # not adjacent


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_restart_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "elmk.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES
    for path in (L.LIB_PATH, L.F32_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW_SYMBOLS:
            assert re.search(r"\bT " + name + r"$", syms, re.M), (path, name)


def test_header_layout_matches_the_codec(tmp_path):
    """sizeof / offsetof of the three structs of elmk.h, compiled with the C compiler, equal restart.py's dtypes."""
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "elmk.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(elmk_restart_header), sizeof(elmk_restart_entry), sizeof(elmk_restart_section),"
                   "offsetof(elmk_restart_header, header_checksum), offsetof(elmk_restart_section, checksum));return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [R.HEADER.itemsize, R.ENTRY.itemsize, R.SECTION.itemsize, R.HEADER.fields["header_checksum"][1],
                   R.SECTION.fields["checksum"][1]]
