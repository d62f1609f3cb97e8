"""The river stage's parts as a whole (api_routing.cpp's table of parts): which public rows exist under every combination of parts, what
a refusal says for the others, that every id reaches its own row, and what enabling and clearing a part does to the device bytes and
to the four budgets.  Everything runs on one context at 65 cells, one past the 64-cell padding (cld = 128: a row offset that is wrong
by a row lands in another row's padding), on a chain (in-degree 1) with nsub = 2."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import inundation_cases as ic
from tests import reservoir_cases as rc
from tests.river_cases import base, context, finite
from tests.run_cases import DT
from tests.support import bits

pytestmark = pytest.mark.gpu

NCELLS, CLD, NSUB = 65, 128, 2
# the rows and the tables of each optional part's allocation (elmk_kernels.h), from the public counts: the scheme's three public rows,
# QSUB and the two flow buffers beside seven derived parameters; the floodplain's three public rows beside VC, ACHN, AF and the profile's
# E_k and VB_k; the reservoirs' three public rows and the natural flow beside CAP, SMIN, C85, BETA and the twelve targets, and MSTART
ROWS_AND_TABLES = {"kinematic": (3 + 1 + 2, 7), "inundation": (3, 3 + 2 * rt.NPROF), "reservoir": (3 + 1, 4 + rt.NMONTH)}


def part_bytes(part):
    """What enabling the part allocates: every region of the allocation starts on a 256-byte boundary."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    nrows, ntab = ROWS_AND_TABLES[part]
    return up(nrows * CLD * 8) + up(ntab * CLD * 8) + (up(CLD * 4) if part == "reservoir" else 0)


@pytest.fixture(scope="module")
def river():
    """The context with the base part on, and every part's inputs: finite, non-zero storages."""
    D = context(base(), None, NCELLS, cell_map=ic.cell_map)
    D.upload("qflx_snwcp_liq", finite(ic.snwcp(0), 2.0e-5))  # (the budgets are to be numbers)
    D.water_balance(DT)
    ddist, area, p0, volr, wh, wt = ic.cell_values(NCELLS, 40 + NCELLS)
    rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(NCELLS, 60 + NCELLS, area, p0, finite(volr) + 1.0, finite(wh) + 2.0, finite(wt) + 3.0, NSUB, DT)
    cap, target, beta, mstart, res, krls = rc.dam_values(NCELLS, 90 + NCELLS)
    down = np.append(np.arange(1, NCELLS), -1).astype(np.int32)
    D.routing_enable(down, ddist, area, rt.EFFVEL, NSUB)
    V = {"down": down, "params": p, "flood": (rdepth, eprof), "dams": (cap, target, beta, mstart),
         "init": {rt.VOLR: volr, rt.QOUT_SUM: np.arange(1.0, NCELLS + 1.0), rt.WH: wh, rt.WT: wt, rt.WF: finite(wf) + 4.0, rt.RES: finite(res) + 5.0,
                  rt.KRLS: krls + 0.25}}
    yield D, V
    D.close()


def enable(D, V, part):
    if part == "kinematic":
        D.routing_kinematic_enable(V["params"])
    elif part == "inundation":
        D.routing_inundation_enable(*V["flood"])
    else:
        D.routing_reservoir_enable(*V["dams"])


def clear(D, part):
    getattr(D, f"routing_{part}_clear")()


def start(D, V, parts):
    """Exactly `parts` on beside the base part, whatever an earlier test left behind, and their init calls made; returns the ids of
    the rows the init calls set."""
    D.history_clear()
    for part in ("reservoir", "inundation", "kinematic"):
        clear(D, part)  # (nothing to free: OK)
    for part in parts:
        enable(D, V, part)
    rows0 = V["init"]
    D.routing_init(rows0[rt.VOLR], rows0[rt.QOUT_SUM])
    ids = [rt.VOLR, rt.QOUT_SUM]
    if "kinematic" in parts:
        D.routing_kinematic_init(rows0[rt.WH], rows0[rt.WT])
        ids += [rt.WH, rt.WT]
    if "inundation" in parts:
        D.routing_inundation_init(rows0[rt.WF])
        ids += [rt.WF]
    if "reservoir" in parts:
        D.routing_reservoir_init(rows0[rt.RES], rows0[rt.KRLS])
        ids += [rt.RES, rt.KRLS]
    return ids


# ---- 1. the row matrix -----------------------------------------------------------------------------------------------------------------
Y = None  # the row exists
R = "row out of range"
K = r"the kinematic-wave scheme is not on \(elmk_routing_kinematic_enable\)"
F = r"the floodplain inundation is not on \(elmk_routing_inundation_enable\)"
# what elmk_cell_history_add_row says for which = -1 .. 13 under every combination of parts (a reservoir row while the reservoirs are
# off is out of range; a row of the scheme or the floodplain names its part, the floodplain's even while the scheme is off)
MATRIX = {
    (): (R, Y, Y, Y, Y, K, K, K, F, F, F, R, R, R, R),
    ("kinematic",): (R, Y, Y, Y, Y, Y, Y, Y, F, F, F, R, R, R, R),
    ("kinematic", "inundation"): (R, Y, Y, Y, Y, Y, Y, Y, Y, Y, Y, R, R, R, R),
    ("kinematic", "reservoir"): (R, Y, Y, Y, Y, Y, Y, Y, F, F, F, Y, Y, Y, R),
    ("kinematic", "inundation", "reservoir"): (R, Y, Y, Y, Y, Y, Y, Y, Y, Y, Y, Y, Y, Y, R),
}


@pytest.mark.parametrize("parts", list(MATRIX), ids=lambda p: "+".join(("base",) + p))
def test_the_rows_of_every_combination(river, parts):
    """Per combination: the init calls' rows come back from their own ids; after one call every which in -1 .. 13 is readable and
    tapeable or refused with the text of its case; cell 64 of every readable row is element 64 of the full read; and the rows that
    differ by construction differ between ids."""
    D, V = river
    for w in start(D, V, parts):
        assert bits(D.routing_read(w)) == bits(V["init"][w]), w
    D.routing(DT)
    full = {}
    for which, why in zip(range(-1, 14), MATRIX[parts]):
        if why is None:
            full[which] = D.routing_read(which)
            assert full[which].shape == (NCELLS,) and bits(D.routing_read(which, cell0=64, n=1)) == bits(full[which][64:]), which
            D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, which, st.HIST_AVG)
        else:
            with pytest.raises(L.ElmkError, match="elmk_routing_read: unknown row$"):
                D.routing_read(which)
            with pytest.raises(L.ElmkError, match=f"elmk_cell_history_add_row: {why}$"):
                D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, which, st.HIST_AVG)
    groups = [(rt.VOLR, rt.QOUT_SUM)] + ([(rt.WH, rt.WT)] if "kinematic" in parts else []) + ([(rt.RES, rt.KRLS, rt.RES_TAKE)] if "reservoir" in parts else [])
    for g in groups:
        assert len({bits(full[w]) for w in g}) == len(g), g
    D.history_clear()


# ---- 2. the lifecycle ------------------------------------------------------------------------------------------------------------------
def test_enable_and_clear_move_the_bytes_by_the_parts_sizes(river):
    """From the base part alone: every optional part on and off twice, the floodplain and the reservoirs in both orders.  An enable adds
    exactly the part's allocation, a clear takes the count back to where the part's enable found it."""
    D, V = river
    start(D, V, ())
    bytes0 = D.device_bytes
    for _ in range(2):
        enable(D, V, "kinematic")
        bytes1 = D.device_bytes
        assert bytes1 - bytes0 == part_bytes("kinematic")
        for first, second in (("inundation", "reservoir"), ("reservoir", "inundation")):
            for _ in range(2):
                enable(D, V, first)
                bytes2 = D.device_bytes
                assert bytes2 - bytes1 == part_bytes(first)
                enable(D, V, second)
                assert D.device_bytes - bytes2 == part_bytes(second)
                clear(D, first)  # (the other one stays)
                assert D.device_bytes - bytes1 == part_bytes(second)
                clear(D, second)
                assert D.device_bytes == bytes1
        clear(D, "kinematic")
        assert D.device_bytes == bytes0


def test_the_four_budgets_equal_the_restatement(river):
    """All four parts on: after the init calls, and again after one call, every budget is the restatement's of the rows the device
    holds, bit for bit; in turn and twice, since the four share the base part's reduction scratch."""
    D, V = river
    start(D, V, ("kinematic", "inundation", "reservoir"))
    rows0 = V["init"]
    zero = np.zeros(NCELLS)
    want = (rt.budget(rows0[rt.VOLR], zero, zero, V["down"]), rt.kinematic_budget(rows0[rt.WH], rows0[rt.WT]), rt.inundation_budget(rows0[rt.WF]),
            rt.reservoir_budget(rows0[rt.RES], zero))
    for after_call in (False, True):
        if after_call:
            D.routing(DT)
            r = {w: D.routing_read(w) for w in range(13)}
            want = (rt.budget(r[rt.VOLR], r[rt.QIN], r[rt.QOUT], V["down"]), rt.kinematic_budget(r[rt.WH], r[rt.WT]), rt.inundation_budget(r[rt.WF]),
                    rt.reservoir_budget(r[rt.RES], r[rt.RES_TAKE]))
            assert r[rt.QOUT][-1] > 0.0 and np.isfinite(np.concatenate(want)).all()
        for _ in range(2):
            got = (D.routing_budget(), D.routing_kinematic_budget(), D.routing_inundation_budget(), D.routing_reservoir_budget())
            for g, h, n in zip(got, want, (3, 2, 1, 2)):
                assert g.shape == (n,) and bits(g) == bits(h)
