"""The river supply limit with reservoirs, on the host (include/elmk.h "reservoirs", D7; irrigation.supply_limit(dam=)): the argument
off and a grid without dams give S3's bits; a dam cell's storage above SMIN is counted, one at or below it and a NaN are not; the
irrigation's shapes, with the 2100-column cell a dam cell; and the chain that motivates it: with a dry channel, a crop cell at a dam is
granted water where the limit without the reservoir grants none, and the routing's D2 then takes that water out of the reservoir."""
import numpy as np

from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from tests import reservoir_cases as rc
from tests.irrigation_supply_cases import cell_map, cell_values, column_rows
from tests.support import bits

NCOLS, NCELLS, NSPD, IDT, THR = 5003, 70, 8, 1800, 0.1


def _case(seed=51):
    m = cell_map(NCOLS, NCELLS, seed, big=(3, 2100), empty=(0, 61, 62, 63, 64, 65, 66), single=(5, 7), free=50)
    area, volr = cell_values(NCELLS, 52)
    rate, nleft, qirr = column_rows(m[0], m[1], NCOLS, NSPD, 53)
    return m, area, volr, rate, nleft, qirr


def test_off_and_without_dams_s3_keeps_its_bits():
    m, area, volr, rate, nleft, qirr = _case()
    want = ir.supply_limit(*m, area, volr, rate, nleft, IDT, THR, np.zeros(NCELLS), qflx_irrig=qirr)
    tab = rt.reservoir_tables(np.zeros(NCELLS), np.zeros((12, NCELLS)), np.zeros(NCELLS), np.zeros(NCELLS, np.int32))
    got = ir.supply_limit(*m, area, volr, rate, nleft, IDT, THR, np.zeros(NCELLS), qflx_irrig=qirr, dam=(tab, np.full(NCELLS, 1.0e12)))
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])


def test_a_dam_cell_counts_its_storage_above_smin():
    """On the irrigation's shapes with dams in cells 0 (empty), 3 (2100 columns), 5 (one column), 8 .. 13 (the edge storages) and every
    third cell: a cell without a dam and a dam at or below SMIN or with a NaN RES keep S3's rows; a dam above SMIN has
    a = (VOLR * (1 - thr) + (RES - SMIN)) - Vc, cell by cell in Python floats."""
    m, area, volr, rate, nleft, qirr = _case()
    cap, target, beta, mstart = rc.supply_dams(NCELLS, 54, placed=(0, 3, 5, 8, 9, 10, 11, 12, 13))
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    res = rc.supply_res(cap, 55)
    res[3] = 0.7 * cap[3]
    plain = ir.supply_limit(*m, area, volr, rate, nleft, IDT, THR, np.zeros(NCELLS), qflx_irrig=qirr)
    rate_d, rows_d = ir.supply_limit(*m, area, volr, rate, nleft, IDT, THR, np.zeros(NCELLS), qflx_irrig=qirr, dam=(tab, res))
    with np.errstate(all="ignore"):
        above = tab["DAM"] & (res - tab["SMIN"] > 0.0)
    assert above[3] and (tab["DAM"] & ~above).any() and np.isnan(res[tab["DAM"]]).any()
    for k in range(4):
        assert bits(rows_d[k][~above]) == bits(plain[1][k][~above]), k
    assert bits(rows_d[ir.DEMAND]) == bits(plain[1][ir.DEMAND]) and bits(rows_d[ir.COMMITTED]) == bits(plain[1][ir.COMMITTED])
    for c in np.nonzero(above)[0]:
        vd, vc = float(rows_d[ir.DEMAND][c]), float(rows_d[ir.COMMITTED][c])
        a = (float(volr[c]) * (1.0 - THR) + (float(res[c]) - float(tab["SMIN"][c]))) - vc
        avail = a if a > 0.0 else 0.0
        want = avail / vd if vd > avail else 1.0
        assert bits(rt._canon(np.array([want]))) == bits(rows_d[ir.RATIO][c:c + 1]), c
    raised = rows_d[ir.RATIO] > plain[1][ir.RATIO]
    assert raised[above].any() and not raised[~above].any() and (rate_d >= rate).sum() >= (plain[0] >= rate).sum()
    assert (rate_d > plain[0]).any()


def test_a_crop_cell_at_a_dam_is_granted_water_from_a_dry_channel():
    """Three cells, each with two checking columns; the channels are dry.  Without the reservoirs nothing is granted anywhere.  With a
    reservoir above SMIN in cell 1 that cell's columns keep their whole rate, the others still get none; and the routing's next call
    takes the applied water out of the reservoir (D2), not out of the dry channel."""
    ptr, col, w = np.array([0, 2, 4, 6]), np.arange(6, dtype=np.int32), np.full(6, 0.5)
    area, volr = np.full(3, 1.0e8), np.zeros(3)
    rate, nleft = np.full(6, 1.0e-4), np.full(6, float(NSPD))
    cap = np.array([0.0, 5.0e8, 5.0e8])
    tab = rt.reservoir_tables(cap, np.full((12, 3), 5.0), np.ones(3), np.zeros(3, np.int32))
    res = np.array([0.0, 2.0e8, 0.04 * 5.0e8])  # cell 2's reservoir is below SMIN
    r0, rows0 = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, IDT, THR, np.zeros(3))
    r1, rows1 = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, IDT, THR, np.zeros(3), dam=(tab, res))
    assert not r0.any() and not rows0[ir.RATIO].any()
    assert (r1[2:4] == rate[2:4]).all() and not r1[[0, 1, 4, 5]].any() and rows1[ir.RATIO].tolist() == [0.0, 1.0, 0.0]
    # the step applies r1; the routing's call then sees QFLX_IRRIG = r1 and a runoff of nothing
    from elmkernels_amd import regrid
    i = regrid.apply_aggregate(ptr, col, w, r1, 0.0)
    rn = np.zeros(3)
    qin = rt.qin_from_rows(ptr, col, w, np.zeros(6), area, qflx_irrig=r1)
    res2, _, take, qin2 = rt.reservoir_prep(res, np.ones(3), qin, area, tab, 0, False, float(IDT), withdrawal=(rn, i))
    want = (i[1] * 0.001) * area[1] * IDT
    assert take[1] == want > 0.0 and res2[1] == res[1] - want and take[0] == 0.0 and take[2] == 0.0
    assert qin[1] < 0.0 and abs(qin2[1]) <= 1.0e-12 * abs(qin[1]) and qin2[0] == qin[0] and qin2[2] == qin[2]
