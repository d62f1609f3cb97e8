"""The irrigation's river supply limit on the host (include/elmk.h "irrigation: river supply limit"): the marker of S0 over the
irrigation's fifty-step chain; irrigation.supply_limit, the restatement the kernel follows, against a plain scalar loop bit for bit
with every case of the statement in one call, and wrong variants of the statement that the same comparison catches; the physics of two
days on cells whose channels hold less than a day's demand, with restatements only; the uniqueness check of
elmk_irrigation_supply_enable as a stand-alone program, plain and under the sanitizers; the header and the bindings.  No GPU."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests.hydrology_cases import column
from tests.irrigation_cases import CHAIN_STEPS, CHAIN_TOD0, generated, smpso_of
from tests.irrigation_supply_cases import CASES, cell_map, cell_values, census, column_rows
from tests.support import ROOT, bits

NAN = float("nan")
U = 2.0 ** -53


# ---- S0: the marker -----------------------------------------------------------------------------------------------------------------
def _took_b(fields, sched, idt, tod):
    """The columns that take branch B in a step, from B's own conditions on what the step reads."""
    f = {k: np.asarray(fields[k]) for k in ("frac_veg_nosno", "elai", "btran")}
    on = (sched >= 0) & (f["frac_veg_nosno"].reshape(-1) != 0) & (f["elai"].astype(np.float64).reshape(-1) > 0.0)
    on &= f["btran"].astype(np.float64).reshape(-1) < 0.999999
    return on & (ir.seconds_since_start(np.maximum(sched, 0), tod) < idt)


@pytest.mark.parametrize("dt", [1800, 14400, 1700], ids=["dt1800", "dt14400_nspd1", "dt1700_no_divisor"])
def test_the_marker_is_exactly_the_check_branch(dt):
    """S0 over the irrigation's fifty-step chain (the oracle's seven wrappers, then irrigation.step): in every step the columns with
    NLEFT == nspd after the step are exactly the columns that took branch B, at dt = 1800 (nspd 8), dt = 14400 (nspd 1: a window of
    one step, so NLEFT is 1 only in the step of the check) and dt = 1700 (14400 / 1700 is no whole number: nspd 9).  Then the chain
    again from the rows and the state saved right after a step in which columns checked: the first step after the restart finds the
    saved NLEFT == nspd, counts it down before it looks, and marks only its own checks."""
    from tests import helpers as H

    n = 300
    cols, scal, soil, sched = generated(n, 900)
    S = H.oracle_state(cols, scal, soil)
    smpso = smpso_of(cols["vtype"])
    nspd = ir.steps_per_day(dt)
    assert nspd == {1800: 8, 14400: 1, 1700: 9}[dt]

    def one_step(s, rows):
        tod = (CHAIN_TOD0 + dt * s) % 86400
        S.timestep7(float(dt))
        fields = {k: np.array(S.fields[k]) for k in ir.READS}
        took = _took_b(fields, sched, dt, tod)
        out, rows = ir.step(fields, rows, sched, float(dt), tod, smpso)
        for k, v in out.items():
            S.fields[k][...] = v
        marked = rows[ir.NLEFT] == float(nspd)
        assert (marked == took).all(), (s, np.nonzero(marked != took)[0][:5])
        return rows, marked

    rows = np.zeros((ir.NROWS, n))
    saved, marks = None, []
    for s in range(CHAIN_STEPS):
        rows, marked = one_step(s, rows)
        marks.append(marked)
        if saved is None and s >= 3 and marked.sum() >= 2:  # right after a check step: the rows through their bytes, the state as it is
            saved = (s, np.frombuffer(rows.tobytes(), np.float64).reshape(rows.shape).copy(), {k: np.array(v) for k, v in S.fields.items()})
    assert saved is not None and sum(int(m.sum()) for m in marks) > n // 4
    s0, rows, fields0 = saved
    assert (rows[ir.NLEFT] == float(nspd)).any()
    for k, v in fields0.items():
        S.fields[k][...] = v
    for s in range(s0 + 1, min(s0 + 13, CHAIN_STEPS)):
        rows, marked = one_step(s, rows)
        assert (marked == marks[s]).all(), ("restarted", s)


# ---- the statement against a scalar loop ---------------------------------------------------------------------------------------------
def _canon(v):
    return v if v == v else NAN


def scalar_loop(ptr, col, w, area, volr, rate, nleft, qirr, idt, thr, unmet, variant=None):
    """S0 - S6 cell by cell and term by term in plain Python floats, written from include/elmk.h and sharing nothing with
    irrigation.supply_limit.  variant: one of the wrong statements of WRONG."""
    ptr, col = [int(v) for v in ptr], [int(v) for v in col]
    w, area, volr, rate, nleft, qirr, unmet = ([float(v) for v in a] for a in (w, area, volr, rate, nleft, qirr, unmet))
    nspd = (14400 + (idt - 1)) // idt
    out = list(rate)
    rows = [[0.0] * len(area) for _ in range(4)]
    for c in range(len(area)):
        D = C = 0.0
        terms = list(range(ptr[c], ptr[c + 1]))
        if variant == "order":
            terms.reverse()
        for k, p in enumerate(terms):
            i = col[p]
            n = nleft[i]
            x = rate[i] * (float(idt) * n)
            checks = n == float(nspd)
            d = x if checks else 0.0
            e = (x if (not checks and n > 0.0) else 0.0) + qirr[i] * float(idt)
            if variant == "no_vc":
                e = 0.0
            if variant == "no_in_flight":
                e = x if (not checks and n > 0.0) else 0.0
            td, tc = w[p] * d, w[p] * e
            D = td if k == 0 else D + td
            C = tc if k == 0 else C + tc
        Vd, Vc = (D * 0.001) * area[c], (C * 0.001) * area[c]
        if variant == "thr_on_vd":
            a = volr[c] - Vc
            Vd = Vd * (1.0 - thr)
        else:
            a = volr[c] * (1.0 - thr) - Vc
        avail = a if a > 0.0 else 0.0
        ratio = avail / Vd if Vd > avail else 1.0
        for p in terms:
            i = col[p]
            if (nleft[i] == float(nspd) or variant == "all_columns") and ratio != 1.0:
                out[i] = _canon(rate[i] * ratio)
        rows[0][c], rows[1][c], rows[2][c] = _canon(Vd), _canon(Vc), _canon(ratio)
        rows[3][c] = _canon(unmet[c] + (Vd - Vd * ratio))
    return np.array(out), np.array(rows)


WRONG = ("no_vc", "no_in_flight", "all_columns", "thr_on_vd", "order")
IDT = 1800


def _statement_case(thr):
    """60 cells over 700 columns: cells 0 and 30 .. 33 empty, cells 5 and 7 of one term, cell 3 of 90 terms, seven columns in no
    cell; the edge storages in cells 8 .. 13; UNMET_SUM already holding something."""
    ncols, ncells = 700, 60
    ptr, col, w = cell_map(ncols, ncells, 41, big=(3, 90), empty=(0, 30, 31, 32, 33), single=(5, 7))
    area, volr = cell_values(ncells, 42, lo=4.0, hi=7.5)
    rate, nleft, qirr = column_rows(ptr, col, ncols, 8, 43)
    unmet = np.random.default_rng(44).uniform(0.0, 1.0e5, ncells)
    return (ptr, col, w, area, volr, rate, nleft, qirr, IDT, thr, unmet), ncols


@pytest.mark.parametrize("thr", [0.0, 0.1])
def test_the_statement_equals_a_scalar_loop_bit_for_bit(thr):
    args, ncols = _statement_case(thr)
    ptr, col, w, area, volr, rate, nleft, qirr, idt, _, unmet = args
    got_rate, got_rows = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, idt, thr, unmet, qflx_irrig=qirr)
    want_rate, want_rows = scalar_loop(*args)
    assert bits(got_rate) == bits(want_rate)
    for k in range(4):
        assert bits(got_rows[k]) == bits(want_rows[k]), k
    have = census(ptr, col, ncols, volr, nleft, rate, 8, got_rows)
    print("census:", have)
    assert all(have[c] > 0 for c in CASES), [c for c in CASES if not have[c]]
    # what the statement says of the edges: a storage that is zero, negative or NaN supplies nothing, an infinite one everything
    for cell, v in zip(range(8, 14), volr[8:14]):
        if got_rows[ir.DEMAND][cell] > 0.0:
            assert got_rows[ir.RATIO][cell] == (1.0 if v == float("inf") else 0.0), (cell, v)
    # only checking columns of limited cells change, and nothing is changed in place
    changed = bits(got_rate) != bits(rate) and np.nonzero(got_rate != rate)[0]
    assert len(changed) > 0 and (nleft[changed] == 8.0).all()
    assert bits(args[5]) == bits(rate) and bits(args[10]) == bits(unmet)
    # the inputs left out: qflx_irrig=None is a QFLX_IRRIG row of zeros
    z_rate, z_rows = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, idt, thr, unmet)
    w_rate, w_rows = scalar_loop(ptr, col, w, area, volr, rate, nleft, np.zeros(ncols), idt, thr, unmet)
    assert bits(z_rate) == bits(w_rate) and bits(z_rows) == bits(w_rows)


@pytest.mark.parametrize("variant", WRONG)
def test_a_wrong_variant_is_caught(variant):
    """The comparison of the test above does not pass a wrong statement: Vc dropped; this step's application dropped from Vc; the
    ratio applied to every column of the cell; thr applied to Vd instead of VOLR; the terms summed in the reverse order."""
    args, _ = _statement_case(0.1)
    ptr, col, w, area, volr, rate, nleft, qirr, idt, thr, unmet = args
    got_rate, got_rows = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, idt, thr, unmet, qflx_irrig=qirr)
    bad_rate, bad_rows = scalar_loop(*args, variant=variant)
    assert bits(got_rate) != bits(bad_rate) or bits(got_rows) != bits(bad_rows)
    if variant == "all_columns":
        assert bits(got_rows) == bits(bad_rows) and bits(got_rate) != bits(bad_rate)  # (only RATE shows it)
    if variant == "order":
        assert np.abs(got_rows[ir.DEMAND] - bad_rows[ir.DEMAND]).max() <= 1.0e-12 * np.abs(got_rows[ir.DEMAND]).max()  # (roundings only)


# ---- the physics, with restatements only ---------------------------------------------------------------------------------------------
def _crop_fields(sat):
    """One loam column per entry of sat (hydrology_cases.column: watsat 0.45, sucsat 200 mm, bsw 5), what irrigation.step reads:
    vegetated, leafy, stressed, thawed, uncapped.  The soil is not stepped: every day's check measures the same deficit."""
    n = len(sat)
    dz = np.array(column(sat=0.3)["dz"] + [1.0] * 5)
    lev = lambda v: np.concatenate([np.zeros(5), v])  # noqa: E731
    f = {"dz": np.tile(lev(dz), (n, 1)), "t_soisno": np.full((n, 20), 280.0)}
    for k, v in (("sucsat", 200.0), ("bsw", 5.0), ("eff_porosity", 0.45)):
        f[k] = np.full((n, 15), v)
    f["h2osoi_liq"] = np.stack([lev(s * 0.45 * dz * 1.0e3) for s in sat])
    root = np.zeros(15)
    root[:8] = [0.25, 0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04]
    f["rootfr"] = np.tile(root, (n, 1))
    f["qflx_rain_grnd"], f["qflx_snwcp_liq"] = np.zeros(n), np.zeros(n)
    f["do_capsnow"], f["frac_veg_nosno"] = np.zeros(n, np.int32), np.ones(n, np.int32)
    f["elai"], f["btran"] = np.full(n, 2.0), np.full(n, 0.3)
    return f


def _chain(limit, volr0, nsteps=96, thr=0.1):
    """irrigation.step -> supply_limit -> routing.qin_from_rows (qrunoff 0, the QFLX_IRRIG row) -> routing.call, nsteps of 1800 s from
    03:00 UTC.  Three outlet cells of four columns each; columns 0 and 1 of a cell pass 06:00 local in step 4, columns 2 and 3 in
    step 5.  ddist = 1e9 m: a cell releases 3.5e-10 of its storage per second, 5e-6 of it in a four-hour window."""
    ncells, dt = 3, 1800
    n = 4 * ncells
    f = _crop_fields([0.2, 0.25, 0.3, 0.35] * ncells)
    sched = np.tile(np.array([3700, 3700, 1900, 1900], np.int32), ncells)
    ptr, col, w = np.arange(0, n + 1, 4), np.arange(n), np.full(n, 0.25)
    area = np.array([1.0e8, 2.0e8, 0.5e8])
    up, kout = rt.upstream_map(np.full(ncells, -1)), np.full(ncells, rt.EFFVEL / 1.0e9)
    rows, unmet, volr = np.zeros((ir.NROWS, n)), np.zeros(ncells), np.array(volr0, dtype=np.float64)
    log = {"volr": [], "demand": [], "qirr": [], "asked": [], "checks": []}
    for s in range(nsteps):
        tod = (3 * 3600 + dt * s) % 86400
        _, rows = ir.step(f, rows, sched, float(dt), tod, -66000.0)
        checks = rows[ir.NLEFT] == 8.0
        log["asked"].append(np.where(checks, rows[ir.RATE], 0.0))  # (the rate the check asked for, before the limit)
        log["checks"].append(checks)
        if limit:
            rate, srows = ir.supply_limit(ptr, col, w, area, volr, rows[ir.RATE], rows[ir.NLEFT], dt, thr, unmet, qflx_irrig=rows[ir.QFLX_IRRIG])
            rows[ir.RATE], unmet = rate, srows[ir.UNMET_SUM]
            log["demand"].append(srows[ir.DEMAND])
        qin = rt.qin_from_rows(ptr, col, w, np.zeros(n), area, qflx_irrig=rows[ir.QFLX_IRRIG])
        volr, _ = rt.call(volr, qin, kout, up, float(dt), 1)
        log["volr"].append(volr)
        log["qirr"].append(rows[ir.QFLX_IRRIG].copy())
    assert not rows[ir.NLEFT].any()  # every window has closed
    return {k: np.array(v) for k, v in log.items()}, unmet, (ptr, col, w, area)


def test_two_days_on_channels_that_hold_less_than_a_days_demand():
    """Three outlet cells whose channels hold 0.5, 0.7 and 0.9 of the first day's demand, two batches of columns per cell that check
    in adjacent steps, two days.  With thr = 0.1 VOLR stays > 0 in every cell and step; with the limit off the same chain drives every
    VOLR below zero.  And the books close: sum(UNMET_SUM) is the demanded volume minus the applied volume.

    The bound, per cell, counted in roundings of the chain (u = 2^-53; every term is >= 0, so a rounding's relative error u applies to
    a partial result no larger than the final one).  Exact arithmetic (fractions) gives demanded = sum over the checks and the cell's
    checking terms of w * RATE_asked * (idt * nspd) * 0.001 * area and applied = sum over the steps and terms of
    w * QFLX_IRRIG * 0.001 * area * dt, both from the doubles the chain held.  Per check with m = 4 terms in the cell:
      Vd         x (1), w * x (1), m - 1 additions, * 0.001 (1), * area (1)          m + 3 roundings of at most u Vd each
      the unmet  Vd * ratio (1), Vd - that (1)                                       2 more
      applied    RATE = RATE * ratio (1), the only rounding between asked and drawn  1 more (QFLX_IRRIG is RATE, nspd times)
    and UNMET_SUM takes one addition per check whose term is not zero (adding +0.0 is exact), each at most u UNMET_SUM.  So
      |UNMET_SUM - (demanded - applied)| <= u ((m + 6) demanded + nchecks UNMET_SUM), times 1.01 for the higher orders."""
    free, _, (ptr, col, w, area) = _chain(False, np.full(3, 1.0e12), nsteps=48)
    day = np.array([float(sum(Fraction(0.25) * Fraction(q) * 1800 * Fraction(0.001) * Fraction(a) for q in free["qirr"][:, 4 * c:4 * c + 4].reshape(-1)))
                    for c, a in enumerate(area)])
    assert (day > 1.0e6).all()
    volr0 = np.array([0.5, 0.7, 0.9]) * day
    on, unmet, _ = _chain(True, volr0)
    off, _, _ = _chain(False, volr0)
    assert (on["volr"] > 0.0).all(), on["volr"].min(axis=0)
    assert (off["volr"].min(axis=0) < 0.0).all()
    # the two batches of a cell checked in adjacent steps, and the second found the first's water committed
    assert on["checks"][4].reshape(3, 4).tolist() == [[True, True, False, False]] * 3
    assert on["checks"][5].reshape(3, 4).tolist() == [[False, False, True, True]] * 3
    assert (unmet > 0.0).all()
    for c in range(3):
        cols_c = slice(4 * c, 4 * c + 4)
        k = Fraction(0.25) * Fraction(0.001) * Fraction(float(area[c]))
        demanded = sum(k * Fraction(float(r)) * (1800 * 8) for r in on["asked"][:, cols_c].reshape(-1))
        applied = sum(k * Fraction(float(q)) * 1800 for q in on["qirr"][:, cols_c].reshape(-1))
        nchecks = int((on["demand"][:, c] > 0.0).sum())
        assert nchecks == 4
        bound = 1.01 * U * ((4 + 6) * float(demanded) + nchecks * float(unmet[c]))
        miss = abs(float(Fraction(float(unmet[c])) - (demanded - applied)))
        print(f"cell {c}: demanded {float(demanded):.6e} applied {float(applied):.6e} unmet {unmet[c]:.6e} miss {miss:.3e} bound {bound:.3e}")
        assert miss <= bound
        assert float(applied) < float(volr0[c])  # never more than the channel held


# ---- the uniqueness check: tests/c/supply_checks.cc ---------------------------------------------------------------------------------
EXPECTED = [
    ("no terms", "-1"), ("one term", "-1"), ("every column once", "-1"), ("columns in no cell", "-1"), ("last column twice", "4"),
    ("first column twice, adjacent", "0"), ("two repeats, the first in term order wins", "2"), ("three times", "1"),
    ("column out of range before a repeat", "-2"), ("column negative before a repeat", "-2"), ("repeat before a column out of range", "0"),
    ("no columns at all", "-1"), ("100000 columns once", "-1"), ("100000 columns and one again", "77"),
    ("csr_check unique on a repeat", "a column in more than one group (or twice in one)"), ("csr_check repeats allowed", "ok"),
    ("csr_check unique, no repeat", "ok"),
]


def _build_and_run(tmp, sanitized):
    exe = str(tmp / ("supply_checks_san" if sanitized else "supply_checks"))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "supply_checks.cc"), "-o", exe]
    if sanitized:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return None, r.stderr.decode()
    # stand-alone: the program has its own main and nothing of it is loaded into Python.  (Leak detection needs ptrace, which a
    # container may deny.)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().splitlines(), ""


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("supply_checks")


def test_the_uniqueness_check_names_the_first_shared_column(tmp):
    lines, err = _build_and_run(tmp, False)
    assert lines is not None, err
    assert [tuple(s.split(": ", 1)) for s in lines] == EXPECTED


def test_the_same_program_under_the_sanitizers(tmp):
    """-fsanitize=address,undefined, run stand-alone: a read or write outside the marks or the map ends the program."""
    lines, err = _build_and_run(tmp, True)
    if lines is None:
        pytest.fail("the host compiler does not link the sanitizers' static runtimes here:\n" + err[-400:])
    assert [tuple(s.split(": ", 1)) for s in lines] == EXPECTED


def test_the_uniqueness_check_is_csr_checks_scan():
    """One scan serves both: csr_check and csr_shared_column call csr_scan, and the marks and the loop exist once in elmk_maps.h."""
    text = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    assert text.count("seen[(size_t)col[p]]++") == 1 and text.count("std::vector<char> seen(") == 1
    for fn in ("inline const char* csr_check(", "inline int64_t csr_shared_column("):
        body = text[text.index(fn):]
        assert "csr_scan<" in body[:body.index("\n}\n")], fn
    assert "hip" not in text.lower().replace("no hip", "")  # host only


# ---- the header and the bindings ----------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("enable", "init", "read", "reset", "clear")


def test_header_constants_bindings_and_pinned_literals():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert "enum { ELMK_IRRSUP_DEMAND = 0, ELMK_IRRSUP_COMMITTED = 1, ELMK_IRRSUP_RATIO = 2, ELMK_IRRSUP_UNMET_SUM = 3 };" in h
    assert (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM) == (0, 1, 2, 3)
    assert (st.IRRSUP_DEMAND, st.IRRSUP_COMMITTED, st.IRRSUP_RATIO, st.IRRSUP_UNMET_SUM, st.IRRSUP_NROWS) == (0, 1, 2, 3, 4)
    assert "/* ---- irrigation: river supply limit ----" in h
    for s in ("S0.", "S1.", "S2.", "S3.", "S4.", "S5.", "S6."):
        assert f" * {s} " in h[h.index("irrigation: river supply limit"):h.index("/* ---- runoff routing")], s
    assert "int elmk_irrigation_supply_enable(elmk_ctx *ctx, double threshold);" in h
    assert "int elmk_irrigation_supply_init(elmk_ctx *ctx, const double *unmet_sum /*[ncells] or NULL*/);" in h
    assert "int elmk_irrigation_supply_read(elmk_ctx *ctx, int which, double *host, int64_t cell0, int64_t n);" in h
    import ctypes as C

    want = {"enable": [C.c_void_p, C.c_double], "init": [C.c_void_p, C.c_void_p], "read": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64],
            "reset": [C.c_void_p], "clear": [C.c_void_p]}
    for name in ENTRY_POINTS:
        assert re.search(rf"^int elmk_irrigation_supply_{name}\(", h, re.M), name
        assert L.SIGNATURES[f"elmk_irrigation_supply_{name}"] == (C.c_int, want[name]), name
        assert hasattr(st.ELMState, f"irrigation_supply_{name}"), name
    hpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    for name in ENTRY_POINTS:
        assert f"elmk_irrigation_supply_{name}(" in hpp, name
    # what this feature leaves alone, literally: the row families, the restart kinds and versions, the routing's and the irrigation's rows
    assert "ELMK_ROWS_IRRIGATION = 4, ELMK_ROWS_NFAMILY = 5" in h and st.ROWS_IRRIGATION == 4
    assert "ELMK_RESTART_HYDROLOGY = 5, ELMK_RESTART_IRRIGATION = 6 };" in h
    assert "#define ELMK_RESTART_VERSION_IRRIGATION 5u" in h and not re.search(r"#define ELMK_RESTART_VERSION_\w+ 6u", h)
    assert R.OPTIONAL[-1] == (6, 5) and R.VERSION_IRRIGATION == 5
    assert "enum { ELMK_ROUTE_VOLR = 0, ELMK_ROUTE_QIN = 1, ELMK_ROUTE_QOUT = 2, ELMK_ROUTE_QOUT_SUM = 3 };" in h
    assert "enum { ELMK_ROUTE_WH = 4, ELMK_ROUTE_WT = 5, ELMK_ROUTE_QSUR = 6 };" in h
    assert "enum { ELMK_IRR_RATE = 0, ELMK_IRR_NLEFT = 1, ELMK_IRR_QFLX_IRRIG = 2 };" in h
    assert re.search(r"#define ELMK_RUN_IRRIGATION 128\b", h) and re.search(r"#define ELMK_RUN_ROUTING 256\b", h)
    assert not re.search(r"#define ELMK_RUN_\w+ 512\b", h)  # no new run flag
    # the kernel stands beside k_ds_lw_norm and k_irrigation is what it was
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_history.hip")).read()
    assert k.index("void k_ds_lw_norm(") < k.index("void k_irrigation_supply(")
    body = k[k.index("void k_irrigation_supply("):]
    assert "atomic" not in body and "__threadfence" not in body and "nontemporal" not in body
    # the documents say what is true now
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "elmk_irrigation_supply_enable" in integ and "### 20.1" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 25\.", design, re.M) and "elmk_irrigation_supply" in design


def test_the_cost_tool_is_built_on_costlib(tmp_path):
    """tests/tools/cost_irrigation_supply.py takes its protocol from costlib and imports without a device and without the library."""
    import sys

    tools = os.path.join(ROOT, "tests", "tools")
    src = open(os.path.join(tools, "cost_irrigation_supply.py")).read()
    assert "import costlib as CL" in src and "CL.back_to_back(" in src and "CL.compare_libraries(" in src
    for copied in ("def back_to_back", "def run_ms", "def schedule", "def spread", "def interleave", "SIGNATURES", "r % 2 == 0 else"):
        assert copied not in src, copied
    code = "import sys, importlib\nsys.path.insert(0, sys.argv[1])\nm = importlib.import_module('cost_irrigation_supply')\nprint('imported', m.COLS_PER_CELL)\n"
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, tools], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "imported 4", r.stderr[-2000:]
    # the records of the first GPU run of the tool
    import json

    recs = [json.loads(s) for s in open(os.path.join(ROOT, "profiles", "r21_irrigation_supply_cost.jsonl"))]
    assert sorted(r["columns"] for r in recs if "limiter_quiet_ms" in r) == [1000000, 10000000]
    assert sorted(r["columns"] for r in recs if "run_step_with_over_without" in r) == [1000000, 10000000]
    assert sum("this_over_parent" in r for r in recs) == 8
