"""Runoff routing without a GPU (include/elmk.h "runoff routing"): the network check of elmkernels_amd/csrc/elmk_maps.h through a
stand-alone program, plain and under the address and undefined-behaviour sanitizers; the numpy restatement's helpers against it;
physical checks of the restatement (a single reservoir, a steady chain, mass closure in exact rational arithmetic, and the same closure
check held against wrong variants of the statement); the header's constants, the bindings and the literals this feature leaves alone."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import restart as R
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests.support import ROOT

U = 2.0 ** -53  # the unit roundoff of fp64


# ---- the network check: tests/c/routing_checks.cc ------------------------------------------------------------------------------------
def ok(nup, npad, *cells):
    return f"ok nup={nup} npad={npad}" + "".join(f" {c}:{','.join(str(u) for u in ups)}" for c, ups in cells)


EXPECTED = [
    ("ncells 0", rt.E_NCELLS),
    ("ncells 2^31", rt.E_NCELLS),
    ("null down", "null argument"),
    ("null ddist", "null argument"),
    ("null area", "null argument"),
    ("down -2", rt.E_RANGE),
    ("down ncells", rt.E_RANGE),
    ("down == self", rt.E_SELF),
    ("2-cycle", rt.E_CYCLE),
    ("cycle of all cells", rt.E_CYCLE),
    ("cycle reached from a tail", rt.E_CYCLE),
    ("cycle reached from two tails, the second after it is marked", rt.E_CYCLE),
    ("nine upstream cells", rt.E_DEGREE),
    ("ddist 0", rt.E_DDIST),
    ("ddist negative", rt.E_DDIST),
    ("ddist NaN", rt.E_DDIST),
    ("ddist inf", rt.E_DDIST),
    ("area negative", rt.E_AREA),
    ("area NaN", rt.E_AREA),
    ("area inf", rt.E_AREA),
    ("area 0", ok(2, 2)),
    # the network's checks come before ddist's, ddist's before area's
    ("bad ddist and bad area", rt.E_DDIST),
    ("self-loop with a bad ddist", rt.E_SELF),
    ("valid small", ok(2, 2, (0, (-1, -1)), (1, (0, -1)), (2, (1, 3)), (3, (-1, -1)))),
    ("exactly eight upstream cells", ok(8, 8, (0, range(1, 9)), (1, [-1] * 8))),
    ("five upstream cells", ok(5, 8, (0, [1, 2, 3, 4, 5, -1, -1, -1]))),
    ("all cells outlets", ok(0, 1, (0, [-1]), (99, [-1]))),
    ("one cell", ok(0, 1, (0, [-1]))),
    ("two trees joining downstream of a visited path", ok(2, 2, (2, (0, 1)), (5, (2, 4)))),
    ("chain of 100000 cells", ok(1, 1, (0, [-1]), (1, [0]), (99999, [99998]))),
    ("reverse chain of 100000 cells", ok(1, 1, (0, [1]), (99998, [99999]), (99999, [-1]))),
]


def _build_and_run(tmp, sanitized):
    exe = str(tmp / ("routing_checks_san" if sanitized else "routing_checks"))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "routing_checks.cc"), "-o", exe]
    if sanitized:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return None, r.stderr.decode()
    # stand-alone: the program has its own main and nothing of it is loaded into Python.  The stack is limited to 256 KiB, so a check
    # that recursed along the chain of 100 000 cells would end the program.  (Leak detection needs ptrace, which a container may deny.)
    r = subprocess.run(["sh", "-c", 'ulimit -s 256 && exec "$0"', exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().splitlines(), ""


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("routing_checks")


def test_every_network_case_returns_the_entry_points_message(tmp):
    lines, err = _build_and_run(tmp, False)
    assert lines is not None, err
    assert [tuple(s.split(": ", 1)) for s in lines] == EXPECTED


def test_the_same_program_under_the_sanitizers(tmp):
    """The second build of the issue: -fsanitize=address,undefined, run stand-alone.  An out-of-range read or write of the marks, the
    in-degrees or the map ends the program."""
    lines, err = _build_and_run(tmp, True)
    if lines is None:
        pytest.fail("the host compiler does not link the sanitizers' static runtimes here:\n" + err[-400:])
    assert [tuple(s.split(": ", 1)) for s in lines] == EXPECTED


def test_the_network_check_needs_no_hip_and_does_not_recurse():
    text = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    body = text[text.index("inline const char* route_check("):]
    assert "route_check(" not in body[len("inline const char* route_check("):]  # (no call of itself)
    assert "hip" not in body.lower() and "elmk_ctx" not in text


# ---- the restatement's helpers against the same cases --------------------------------------------------------------------------------
def _forest(n, rng, p_outlet=0.03, span=40):
    """A random forest: every cell drains into a later cell within `span`, or is an outlet; at most 8 cells drain into one."""
    down = np.full(n, -1, np.int32)
    deg = np.zeros(n, np.int64)
    for c in range(n - 1):
        if rng.random() < p_outlet:
            continue
        d = int(rng.integers(c + 1, min(c + 1 + span, n)))
        if deg[d] < rt.MAXUP:
            down[c] = d
            deg[d] += 1
    return down


def test_check_network_and_upstream_map_agree_with_the_host_check():
    for down, text in (([1, -2, -1, 2], rt.E_RANGE), ([1, 4, -1, 2], rt.E_RANGE), ([1, 2, -1, 3], rt.E_SELF), ([1, 0, -1, 2], rt.E_CYCLE),
                       ([1, 2, 3, 0], rt.E_CYCLE), ([1, 2, 3, 4, 2, -1], rt.E_CYCLE), ([3, 3, 4, 4, 5, 3, 0], rt.E_CYCLE),
                       ([-1] + [0] * 9, rt.E_DEGREE), ([], rt.E_NCELLS)):
        with pytest.raises(ValueError, match=re.escape(text)):
            rt.check_network(np.array(down, np.int32))
    with pytest.raises(ValueError, match=re.escape(rt.E_DDIST)):
        rt.check_network([1, -1], ddist=[1.0, 0.0], area=[np.nan, 1.0])
    with pytest.raises(ValueError, match=re.escape(rt.E_AREA)):
        rt.check_network([1, -1], ddist=[1.0, 2.0], area=[-1.0, 1.0])
    rt.check_network([-1] + [0] * 8, ddist=np.ones(9), area=np.zeros(9))
    rt.check_network(np.append(np.arange(1, 100000), -1))  # (a loop, not a recursion)
    up = rt.upstream_map([1, 2, -1, 2])
    assert up.shape == (8, 4) and up.dtype == np.int32
    assert up[:2].tolist() == [[-1, 0, 1, -1], [-1, -1, 3, -1]] and (up[2:] == -1).all()
    assert rt.upstream_map([-1] + [0] * 8)[:, 0].tolist() == list(range(1, 9)) and rt.npad_of(rt.upstream_map([-1] + [0] * 8)) == 8
    assert [rt.npad_of(rt.upstream_map([-1] + [0] * k)) for k in range(9)] == [1, 1, 2, 4, 4, 8, 8, 8, 8]
    rng = np.random.default_rng(5)
    down = _forest(1001, rng)
    rt.check_network(down)
    up = rt.upstream_map(down)
    for c in range(1001):  # the definition: the cells u with down[u] == c in ascending u, padded with -1
        want = np.nonzero(down == c)[0].tolist()
        assert up[:, c].tolist() == want + [-1] * (8 - len(want))


def test_d8_network():
    # a 3 x 4 grid: everything drains east along each row, the last column south, the south-east corner is the outlet
    d = np.array([[1, 1, 1, 4], [1, 1, 1, 4], [1, 1, 1, 0]])
    down = rt.d8_network(3, 4, d)
    assert down.dtype == np.int32 and down.tolist() == [1, 2, 3, 7, 5, 6, 7, 11, 9, 10, 11, -1]
    # a direction that leaves the grid makes an outlet; the diagonals
    assert rt.d8_network(2, 2, [[32, 128], [8, 2]]).tolist() == [-1, -1, -1, -1]
    assert rt.d8_network(2, 2, [[2, 0], [0, 0]]).tolist() == [3, -1, -1, -1]
    with pytest.raises(ValueError, match=re.escape(rt.E_CYCLE)):
        rt.d8_network(1, 2, [[1, 16]])


# ---- R2 and the flow's edge values ---------------------------------------------------------------------------------------------------
def test_flow_edge_values():
    k, dts = 1.0e-4, 900.0
    v = np.array([0.0, -0.0, -5.0, np.nan, -np.inf, 5e-324, 1.0, 1e300, np.inf])
    f = rt.flow(v, k, dts)
    assert f[:5].tolist() == [0.0] * 5 and not np.signbit(f[:5]).any()  # a NaN, zero, negative-zero or negative storage releases +0.0
    assert f[5] == 0.0 and f[6] == 1.0e-4 and f[7] == 1e300 * k and f[8] == np.inf
    # the cap: k * dts >= 1 releases v / dts, exactly what the cell holds
    assert rt.flow(np.array([90.0]), 0.5, 900.0)[0] == 0.1 and rt.flow(np.array([90.0]), 1.0 / 900.0, 900.0)[0] == 90.0 * (1.0 / 900.0)


# ---- physical checks of the restatement ----------------------------------------------------------------------------------------------
def test_single_reservoir_decays_geometrically():
    """No input: v_n = v0 (1 - k dts)^n.  A sub-step takes 3 roundings (v * k, * dts, the final sum; fin - f = 0 - f and + QIN = + 0 are
    exact): v' = v - v x (1 + e1)(1 + e2), then (1 + e3), x = k dts, so one sub-step's relative error is at most
    u (1 + 2 x / (1 - x)) to first order and n sub-steps' at most n times that; the bound allows 1 % for the higher orders.  The
    reference is exact rational arithmetic on the doubles k and dts."""
    up = rt.upstream_map([-1])
    for k, dt, nsub, ncall in ((0.35 / 5000.0, 1800.0, 1, 200), (0.35 / 2000.0, 1800.0, 7, 40), (0.35 / 700.0, 1800.0, 2, 30)):
        v0 = 123456.789
        v = np.array([v0])
        for _ in range(ncall):
            v, q = rt.call(v, np.zeros(1), np.array([k]), up, dt, nsub)
        dts = dt / nsub
        x = k * dts
        assert 0.0 < x < 1.0
        n = nsub * ncall
        exact = Fraction(v0) * (1 - Fraction(k) * Fraction(dts)) ** n
        err = abs(Fraction(float(v[0])) - exact) / exact
        bound = 1.01 * n * U * (1.0 + 2.0 * x / (1.0 - x))
        print(f"single reservoir: k dts {x:.3f}, {n} sub-steps: relative error {float(err):.3e}, bound {bound:.3e}")
        assert err <= bound


def test_a_chain_with_constant_input_reaches_the_steady_state():
    """QOUT of the last cell of a chain tends to the sum of the inputs: the deficit shrinks by the slowest cell's factor (1 - k dts) per
    sub-step, here 0.37 at the most, so 400 calls leave nothing of it beside the rounding of ten additions."""
    n = 10
    down = np.append(np.arange(1, n), -1).astype(np.int32)
    up = rt.upstream_map(down)
    ddist = np.linspace(1000.0, 2000.0, n)
    kout = rt.EFFVEL / ddist
    qin = np.linspace(0.5, 5.0, n)
    v = np.zeros(n)
    last = []
    for _ in range(400):
        v, q = rt.call(v, qin, kout, up, 1800.0, 2)
        last.append(q[-1])
    assert (np.diff(last[:50]) > 0.0).all()  # it rises to it
    assert abs(last[-1] - qin.sum()) <= 32 * U * qin.sum()
    assert np.abs(v * kout - np.cumsum(qin)).max() <= 64 * U * qin.sum()  # every cell passes on what arrives above it


def _closure_inputs(seed):
    rng = np.random.default_rng(seed)
    n = 1001
    down = _forest(n, rng)
    ddist = np.exp(rng.uniform(np.log(500.0), np.log(60000.0), n))  # 500 m .. 60 km: k dts > 1 below 630 m at dts = 1800 s
    short = rng.random(n) < 0.03
    ddist[short] = rng.uniform(40.0, 85.0, int(short.sum()))  # and a few short reaches, capped at dts = 1800 / 7 s as well (below 90 m)
    kout = rt.EFFVEL / ddist
    area = rng.uniform(0.5e8, 2.5e8, n)
    v0 = rng.uniform(0.0, 1.0e6, n)
    qins = [(rng.uniform(0.0, 2.0e-5, n) * 0.001) * area for _ in range(50)]
    return down, kout, v0, qins


def _fsum(x):
    return sum((Fraction(float(a)) for a in x), Fraction(0))


def _closure(down, kout, v0, qins, dt, nsub, **variant):
    """50 calls; returns (the largest |residual| of a call, the sum of the calls' bounds, mean sum |VOLR|, cap hits).  The residual of
    one call, in exact rational arithmetic on the doubles: sum(VOLR_end) - sum(VOLR_beg) - dt (sum QIN - sum outlet QOUT).

    The bound.  In real arithmetic a sub-step moves every flow from one cell to the next or out of an outlet, so it conserves the sum.
    What is computed differs by the roundings of R3 - R4, at most 12 per cell and sub-step (8 additions into fin, fin - f, + QIN,
    * dts, the final sum), each at most u times the magnitude of what it rounds, which is at most |v| + (fin + f + |QIN|) dts; the cap
    gives f dts <= v and fin dts <= the upstream cells' storages, so summed over the cells that is at most 3 sum |v| + dts sum |QIN|.
    With storages and inputs that are not negative the sum of the storages inside a call is at most its start's plus dt sum QIN.  R5
    rounds the outlets' flow sum nsub times and its mean once, each at most u times a flow that, times dt, is at most nsub times the
    outlet's storage; and dts nsub differs from dt by u dt.  Hence per call
        u (12 nsub (3 SV + dts SQ) + (nsub + 1) nsub SVO + dt (SQ + SO)),   SV = sum |v| at the start + dt SQ, SQ = sum |QIN|,
        SO = sum outlet QOUT, SVO = SV (the outlets hold no more than everything)."""
    up = rt.upstream_map(down)
    v = v0.copy()
    dts = dt / nsub
    worst, bound, mags, hits = Fraction(0), 0.0, [], 0
    total = Fraction(0)
    for qin in qins:
        hits += int(((v > 0.0) & (kout * dts > 1.0)).sum())
        v1, qout = rt.call(v, qin, kout, up, dt, nsub, **variant)
        so = _fsum(qout[down < 0])
        res = _fsum(v1) - _fsum(v) - Fraction(dt) * (_fsum(qin) - so)
        total += res
        worst = max(worst, abs(total))
        sq = float(np.abs(qin).sum())
        sv = float(np.abs(v).sum()) + dt * sq
        bound += U * (12 * nsub * (3 * sv + dts * sq) + (nsub + 1) * nsub * sv + dt * (sq + float(so)))
        mags.append(float(np.abs(v1).sum()))
        v = v1
    return float(worst), bound, float(np.mean(mags)), hits, v


@pytest.mark.parametrize("nsub", [1, 7])
def test_mass_closure_in_exact_arithmetic_and_the_wrong_variants(nsub):
    """Over 50 calls on a random forest of 1001 cells the accumulated residual stays below the bound of _closure.  Measured
    (accumulated over the 50 calls, beside the bound, as a fraction of the mean sum |VOLR|):
        nsub 1: residual 1.7e-17, bound 2.1e-13;  nsub 7: residual 6.1e-17, bound 1.7e-12    (cap reached 4200 / 1750 times)
    and for the wrong variants, in bounds: in place 1.1e13 / 3.1e11, upstream flows uncapped 6.9e12 / 5.8e10, no cap at all 5e-4 / 3e-5.
    The same check held against wrong statements must exceed the bound by at least 1e3, or the input tests nothing:
      - in place: cells updated one after another, the flows of R3 taken from storages already updated in the sub-step;
      - the cap dropped from the upstream flows of R3 where k dts > 1 while the cell's own release keeps it (the slip a kernel that
        evaluates the upstream flows again can make).
    Dropping the cap from every flow alike moves the same water out of one cell and into the next, so no closure check can see it (its
    residual is printed: it stays under the bound); what it breaks is that a storage fed by inputs that are not negative never goes
    below zero by more than the rounding of its own update, which is asserted for the statement and fails for that variant by the
    storages' own magnitude."""
    dt = 1800.0
    down, kout, v0, qins = _closure_inputs(20 + nsub)
    res, bound, mag, hits, v_end = _closure(down, kout, v0, qins, dt, nsub)
    print(f"closure, nsub {nsub}: residual {res:.3e} m3 = {res / mag:.2e} of the mean sum |VOLR|; bound {bound:.3e} = {bound / mag:.2e}; cap reached {hits} times")
    assert hits >= 50
    assert res <= bound
    assert v_end.min() >= -4 * U * v0.max()
    ip = _closure(down, kout, v0, qins[:5], dt, nsub, in_place=True)
    up_only = _closure(down, kout, v0, qins, dt, nsub, cap="own")
    nocap = _closure(down, kout, v0, qins, dt, nsub, cap=False)
    print(f"  in place: residual {ip[0]:.3e} ({ip[0] / ip[1]:.1e} bounds); upstream flows uncapped: {up_only[0]:.3e} ({up_only[0] / up_only[1]:.1e} bounds); "
          f"no cap at all: residual {nocap[0]:.3e} ({nocap[0] / nocap[1]:.1e} bounds), lowest storage {nocap[4].min():.3e}")
    assert ip[0] >= 1.0e3 * ip[1]
    assert up_only[0] >= 1.0e3 * up_only[1]
    assert nocap[4].min() <= -1.0e3 * 4 * U * v0.max()


def test_qin_and_budget_restatements():
    from elmkernels_amd import diagnostics, regrid

    rng = np.random.default_rng(3)
    ncols, ncells = 50, 12
    cell = rng.integers(-1, ncells - 1, ncols)  # (the last cell has no columns)
    ptr, col, w = regrid.owner_map(cell, rng.uniform(1.0, 2.0, ncols), ncells)
    q, irr = rng.uniform(-1e-5, 1e-4, ncols), rng.uniform(0.0, 1e-5, ncols)
    area = rng.uniform(1e7, 1e8, ncells)
    qin = rt.qin_from_rows(ptr, col, w, q, area)
    r = regrid.apply_aggregate(ptr, col, w, q, 0.0)
    assert np.array_equal(qin, (r * 0.001) * area) and qin[-1] == 0.0 and not np.signbit(qin[-1])
    wd = rt.qin_from_rows(ptr, col, w, q, area, qflx_irrig=irr)
    assert np.array_equal(wd, ((r - regrid.apply_aggregate(ptr, col, w, irr, 0.0)) * 0.001) * area)
    q[3] = np.nan
    assert np.isnan(rt.qin_from_rows(ptr, col, w, q, area)[cell[3]]) if cell[3] >= 0 else True
    down = np.array([1, 2, -1, -1] + [3] * 8, np.int32)
    b = rt.budget(area, qin, area * 2.0, down)
    assert b[0] == diagnostics.reduce_min_max_sum(area)[2] and b[1] == diagnostics.reduce_min_max_sum(qin)[2]
    assert b[2] == 2.0 * area[2] + 2.0 * area[3]


# ---- the header, the bindings and the literals that stay ----------------------------------------------------------------------------
ENTRY_POINTS = ("enable", "init", "read", "count", "reset_mean", "set_withdrawal", "budget", "clear")


def test_header_constants_bindings_and_pinned_literals():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert re.search(r"#define ELMK_RUN_ROUTING 256\b", h) and st.RUN_ROUTING == 256
    assert "enum { ELMK_ROUTE_VOLR = 0, ELMK_ROUTE_QIN = 1, ELMK_ROUTE_QOUT = 2, ELMK_ROUTE_QOUT_SUM = 3 };" in h
    assert (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM) == (st.ROUTE_VOLR, st.ROUTE_QIN, st.ROUTE_QOUT, st.ROUTE_QOUT_SUM) == (0, 1, 2, 3)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int elmk_routing_{name}\(", h, re.M) and f"elmk_routing_{name}" in L.SIGNATURES, name
    assert "int elmk_routing(elmk_ctx *ctx, double dt);" in h and "elmk_routing" in L.SIGNATURES
    assert "/* ---- runoff routing ----" in h
    for name in ENTRY_POINTS + ("",):
        assert hasattr(st.ELMState, "routing" + ("_" + name if name else ""))
    # what this feature leaves alone: the image format, the restart kinds and the row families
    assert "ELMK_ROWS_IRRIGATION = 4, ELMK_ROWS_NFAMILY = 5" in h
    assert "ELMK_RESTART_HYDROLOGY = 5, ELMK_RESTART_IRRIGATION = 6 };" in h
    assert "#define ELMK_RESTART_VERSION_IRRIGATION 5u" in h and not re.search(r"#define ELMK_RESTART_VERSION_\w+ 6u", h)
    assert R.OPTIONAL[-1] == (6, 5) and R.VERSION_IRRIGATION == 5
    assert re.search(r"#define ELMK_RUN_IRRIGATION 128\b", h) and re.search(r"#define ELMK_RUN_WATER_BALANCE 64\b", h)
    # the documents say what is modelled now
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "water withdrawal is not modelled" not in integ.lower()
    assert "elmk_routing_set_withdrawal" in integ and "elmk_routing_init" in integ


def test_the_units_are_last_in_the_makefile():
    mk = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KSRC\s*:=.* k_routing\.hip$", mk, re.M) and re.search(r"^HOSTSRC\s*:=.* api_routing\.cpp$", mk, re.M)
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_routing.hip")).read()
    assert "nontemporal_" not in k and "atomic" not in k.replace("no atomics", "") and "__threadfence" not in k


def test_the_cost_tool_is_built_on_costlib(tmp_path):
    """tests/tools/cost_routing.py takes its protocol from costlib (no copy of a helper, no symbol table of its own) and imports without
    a device and without the built library, as tests/test_cost_tools_host.py asks of the *_cost.py tools."""
    import sys

    tools = os.path.join(ROOT, "tests", "tools")
    src = open(os.path.join(tools, "cost_routing.py")).read()
    assert "import costlib as CL" in src and "CL.back_to_back(" in src and "CL.run_ms(" in src and "CL.compare_libraries(" in src
    for copied in ("def back_to_back", "def run_ms", "def schedule", "def spread", "def interleave", "SIGNATURES", "r % 2 == 0 else"):
        assert copied not in src, copied
    code = "import sys, importlib\nsys.path.insert(0, sys.argv[1])\nm = importlib.import_module('cost_routing')\nprint('imported', m.CALLS)\n"
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, tools], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "imported 40", r.stderr[-2000:]
    # the records of the first GPU run of the tool
    import json

    recs = [json.loads(s) for s in open(os.path.join(ROOT, "profiles", "r19_routing_cost.jsonl"))]
    assert sorted(r["cells"] for r in recs if "launches" in r) == [10000, 200000, 4000000]
    assert sorted(r["columns"] for r in recs if "run_step_with_over_without" in r) == [1000000, 10000000]
    assert sum("this_over_parent" in r for r in recs) == 8
