"""The generated tier of the irrigation tests, host and device: columns that take every branch of the stage over fifty chained steps,
the chain's times of day, and the plant types' smpso."""
import os

import numpy as np

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H

CHAIN_STEPS = 50  # 1800 s steps: a day and two steps
CHAIN_TOD0 = 3 * 3600


def chain_tod(s):
    return (CHAIN_TOD0 + 1800 * s) % 86400


def generated(n, seed):
    """The branch-mix generator's columns (synth.make_state, tier B) arranged so that fifty chained steps of the seven wrappers and the
    stage take every branch of A and B: longitudes every half hour of local time with a few hundred seconds of scatter, so that inside
    one wave some columns check, some apply and some do neither; one column in nine not irrigated; bare and leafless columns; capped
    columns; columns frozen at the top (their window opens at rate +0.0) and below layer 3; saturated columns (unstressed) and columns
    wet on top and dry below (deficit 0 beside deficit > 0); roots in the ten active layers only.  Returns (cols, scal, soil, sched)."""
    cols, scal, soil = synth.make_state(st.field_table() if os.path.exists(L.LIB_PATH) else H.field_table_from_oracle(), n, tier="B", seed=seed)
    c = np.arange(n)
    rng = np.random.default_rng(seed + 5)
    s0 = 5
    dzmm = cols["dz"][:, s0:s0 + 15] * 1.0e3
    watsat = cols["watsat"]
    cols["t_soisno"][:, s0:] = np.maximum(cols["t_soisno"][:, s0:], 276.0)  # thawed, unless set otherwise below
    cols["h2osoi_ice"][:, s0:] = 0.0
    root = rng.uniform(0.02, 1.0, (n, 15))
    root[:, 10:] = 0.0
    root[c % 4 == 1, 1] = 0.0
    cols["rootfr"] = root / root.sum(axis=1, keepdims=True)
    cols["h2osoi_liq"][:, s0:] = rng.uniform(0.15, 0.5, (n, 15)) * watsat * dzmm
    m = c % 7 == 2  # saturated: btran reaches 1
    cols["h2osoi_liq"][m, s0:] = watsat[m] * dzmm[m]
    m = c % 7 == 3  # wet on top, dry below
    cols["h2osoi_liq"][m, s0:s0 + 3] = 0.98 * watsat[m, :3] * dzmm[m, :3]
    cols["t_soisno"][c % 6 == 4, s0] = 272.0  # frozen at the top
    cols["t_soisno"][c % 6 == 5, s0 + 3] = 270.0  # frozen layer 3
    cols["frac_veg_nosno"][:] = np.where(c % 10 == 6, 0, 1)
    cols["frac_veg_nosno_alb"][:] = cols["frac_veg_nosno"]
    cols["elai"][:] = np.where(c % 10 == 8, 0.0, np.maximum(cols["elai"], 0.3))
    cols["esai"][:] = np.maximum(cols["esai"], 0.1)
    cols["do_capsnow"][:] = (c % 5 == 0).astype(np.int32)
    lon = ((c * 7) % 48) * 7.5 - 180.0 + (c % 9) * 0.4  # 0.4 degrees = 96 s
    sched = ir.schedule(c % 9 != 4, lon)
    return cols, scal, soil, sched


def smpso_of(vtype):
    pft, _ = synth.load_params()
    return np.asarray(pft["smpso"], dtype=np.float64).reshape(-1)[np.asarray(vtype)]
