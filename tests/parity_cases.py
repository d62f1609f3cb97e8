"""The states the device parity tests feed the kernels, in one list.

Each case names a tier, a size, a seed, a land unit, overrides of the context scalars and how many steps of which chain
run on it.  The GPU tests of tier W (tests/test_gpu_wide.py) take their states from here, and the oracle coverage test
(tests/test_oracle_coverage.py) replays this list through the oracle with the same chain definition (oracle_step) the
tier-W GPU tests drive the oracle with: the coverage it reports is that of what the device is checked on.

Chains: "step7" = the seven wrappers; "advance" = init_timestep, the seven, soil_temperature, snow_hydrology, surface_fluxes
and the conservation diagnostics (ELMInterface::advance's device part); "snow" = the seven and soil_temperature, then snow_hydrology once.
"""
from dataclasses import dataclass, field

from elmkernels_amd import synth

DT = 1800.0

WETLAND = dict(ltype=6, ctype=0, vtype=0, urbpoi=0, lakpoi=0)
ICE = dict(ltype=3, ctype=0, vtype=0, urbpoi=0, lakpoi=0)
URBAN = dict(ltype=7, ctype=71, vtype=0, urbpoi=1, lakpoi=0)
CROP = dict(ltype=2, ctype=0, vtype=15, urbpoi=0, lakpoi=0)
OTHER_LANDS = (WETLAND, ICE, URBAN, CROP)
# land units only tier W runs: a deep lake, and the urban columns other than the roof (walls, pervious and impervious road)
DEEP_LAKE = dict(ltype=5, ctype=0, vtype=0, urbpoi=0, lakpoi=1)
URBAN_PARTS = tuple(dict(ltype=7, ctype=ct, vtype=0, urbpoi=1, lakpoi=0) for ct in (72, 73, 74, 75))

# context-wide scalars the fixtures never vary (they hold oldfflag = 0, dewmx = 0.1, dayl = max_dayl = 86400.0001)
OLDFFLAG = dict(oldfflag=1)
DEWMX = dict(dewmx=0.037)
SHORT_DAY = dict(dayl=31000.0, max_dayl=52000.0)
# what a context holds when elmk_set_scalars is never called (elmk_api.cpp: the reference's ELMState defaults)
ABI_DEFAULT = dict(dewmx=0.1, oldfflag=1, dayl=0.0, max_dayl=0.0)


@dataclass(frozen=True)
class Case:
    name: str
    tier: str
    n: int
    seed: int
    steps: int = 1
    chain: str = "step7"
    land: dict = None
    scalars: dict = field(default_factory=dict)


# the states of the main tier A / B parity tests of tests/test_gpu_parity.py, restated here for the coverage replay (those tests
# keep their own parameters: this list is a copy of them, not their source, and is kept in step with them by hand)
EXISTING = [
    Case("A_chain", "A", 4700, 11, steps=2),
    Case("B_chain", "B", 20000, 42, steps=3),
    Case("B_snow", "B", 20000, 42, chain="snow"),
    Case("B_advance", "B", 6016, 14, steps=12, chain="advance"),
    Case("B_small", "B", 1001, 43, chain="snow"),
] + [Case(f"B_land{k}", "B", 2000 + 1000 * (k % 2), 21 + 23 * (k % 2), chain="snow", land=land)
     for k, land in enumerate(OTHER_LANDS)]

# tier W: the wide draw with its edge rows, on its own and under each context-scalar variant
WIDE = [
    Case("W_wrappers", "W", 4096, 7, steps=2),
    Case("W_advance", "W", 3008, 8, steps=12, chain="advance"),
    Case("W_oldfflag", "W", 2048, 9, steps=4, chain="advance", scalars=OLDFFLAG),
    Case("W_dewmx", "W", 2048, 10, steps=2, scalars=DEWMX),
    Case("W_short_day", "W", 2048, 11, steps=2, scalars=SHORT_DAY),
    Case("W_abi_default", "W", 2048, 12, steps=2, scalars=ABI_DEFAULT),
] + [Case(f"W_land{k}", "W", 2048, 13 + k, steps=4, chain="advance", land=land)
     for k, land in enumerate(OTHER_LANDS + (DEEP_LAKE,) + URBAN_PARTS)]

CASES = EXISTING + WIDE
BY_NAME = {c.name: c for c in CASES}


def state(case, field_table):
    """-> (columns, scalars, soil-colour tables) of the case, scalars with the case's overrides applied."""
    cols, scal, soil = synth.make_state(field_table, case.n, tier=case.tier, seed=case.seed)
    return cols, dict(scal, **case.scalars), soil


HEIGHTS = ("forc_hgt_u_patch", "forc_hgt_t_patch", "forc_hgt_q_patch")


def heights(S):
    """The forcing heights of a fresh state: the driver puts them back before every step (atm_physics_impl.hh:197-203),
    because canopy_temperature adds the roughness length and displacement height to them."""
    return {k: S[k].copy() for k in HEIGHTS}


def oracle_step(S, case, hgt, dt=DT):
    """One step of the case's chain on an oracle state (hgt: heights(S) of the start state)."""
    for k, v in hgt.items():
        S[k][...] = v
    if case.chain == "advance":
        S.init_timestep()
    S.timestep7(dt)
    if case.chain in ("advance", "snow"):
        S.soil_temperature(dt)
        S.snow_hydrology(dt)
    if case.chain == "advance":
        S.surface_fluxes(dt)
        S.evaluate_conservation(dt)


def replay(case, field_table=None):
    """The case's whole chain on the oracle (a "snow" case: one step); returns the final state."""
    from tests import helpers as H

    cols, scal, soil = state(case, field_table or H.field_table_from_oracle())
    S = H.oracle_state(cols, scal, soil, case.land)
    hgt = heights(S)
    for _ in range(1 if case.chain == "snow" else case.steps):
        oracle_step(S, case, hgt)
    return S
