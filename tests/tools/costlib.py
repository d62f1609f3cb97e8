"""The measuring protocol of the tests/tools/*_cost.py tools, once.

Writing a cost tool.  Start from this module, not from a copy of another tool.  A tool is a docstring that names its modes and byte
tallies, a `build` that takes `run_context` (or `base_context`) and enables its feature, a `measure(cols, rounds, ...)` that returns one
JSON-serialisable record, and a `main` made of `cli` and `emit_each`.  Inside `measure`, time a launch with `back_to_back` and a run
step with `run_ms`; let the modes of a round take their turns in the order `interleave(r, keys)` gives, and reduce the per-mode lists
with `medians` and `spreads`.  To set this build beside another build of the library (the parent commit's, a variant) use
`compare_libraries`: it loads the builds, creates one context per build in one process, gives them turns, and closes them.  The repeat
counts are arguments because they decide whether two records can be compared: pass them, and name them in the tool's docstring.
What belongs to one feature - byte tallies, tiers, geographies, what is reset before a series - stays in its tool.

A tool puts this directory on sys.path and imports the module:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import costlib as CL"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from elmkernels_amd import _lib as L  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = 1800.0
FORC, PHEN = st.SERIES_FORCING, st.SERIES_PHENOLOGY


# ---- contexts ----

def base_context(cols, tier="A", lib_path=None, geography=None):
    """The benchmark's state with the snow-age tables and graphs on.  geography: None, a seed of synth.global_grid, or (lat, lon)."""
    D, _ = bench.build_state(cols, 0, tier, 0x5EEDE1A0, lib_path=lib_path)
    D.set_snow_age_tables(synth.snow_age_tables())
    D.set_graph(True)
    if geography is not None:
        lat, lon = geography if isinstance(geography, tuple) else synth.global_grid(cols, seed=geography)
        D.set_column_geography(lat, lon)
    return D


def resident_records(D, slots=2, max_steps=64, records=None):
    """Reserve a run and make its series resident.  records None: the two forcing records and two months the state already holds, as they
    are.  records n: n forcing records and twelve months, alternating between the state's two rows."""
    D.run_reserve(slots, max_steps)
    if records is None:
        for k in FORC + PHEN:
            D.series_upload(k, 0, D.download(k, layout=st.LAYOUT_SOA))
        return
    for k in FORC:
        a = D.download(k, layout=st.LAYOUT_SOA)
        for r in range(records):
            D.series_upload(k, r, a[r % 2])
    for k in PHEN:
        a = D.download(k, layout=st.LAYOUT_SOA)
        D.series_upload(k, 0, np.stack([a[m % 2] for m in range(12)]))


def run_context(cols, tier="A", lib_path=None, geography_seed=11, slots=2, max_steps=64, records=None):
    """A context elmk_run can step: base_context over a global grid, then resident_records.  The defaults are the tier-A form of the
    feature tools; the tier-B form has geography_seed None (synth.global_grid's own seed) and slots = records = its record count."""
    D = base_context(cols, tier, lib_path, synth.global_grid(cols) if geography_seed is None else geography_seed)
    resident_records(D, slots, max_steps, records)
    return D


def load_build(path, optional=()):
    """Another build of the library (the parent commit's, a variant).  optional: name prefixes of entry points it may lack."""
    return L.load(path, optional=optional)


# ---- schedules ----

def schedule(n):
    """n half-hour steps inside one forcing bracket (slot 0) and one month bracket: the run over the two records a state holds."""
    S = np.zeros(n, st.RUN_STEP_DTYPE)
    for s in range(n):
        ddoy = 180.25 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), 0
        w2 = np.full(8, (s + 0.5) / n)
        S[s]["forc_wt1"], S[s]["forc_wt2"] = 1.0 - w2, w2
        S[s]["month1"], S[s]["month2"], S[s]["month_wt1"], S[s]["month_wt2"] = 0, 1, 0.6, 0.4
    return S


def evolving_schedule(n, day0, steps_per_record, months):
    """n half-hour steps from day of year day0 that walk the forcing records, steps_per_record steps to a bracket, the eight streams'
    weights 0.03 apart.  months: (month1, month2) for every step, or one pair per step; the month weights are 0.4 and 0.6."""
    S = np.zeros(n, st.RUN_STEP_DTYPE)
    pairs = [months] * n if isinstance(months[0], int) else months
    for s in range(n):
        ddoy = day0 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), s // steps_per_record
        w2 = np.clip(((s % steps_per_record) / steps_per_record) + 0.03 * np.arange(8), 0.0, 1.0)
        S[s]["forc_wt2"], S[s]["forc_wt1"] = w2, 1.0 - w2
        (S[s]["month1"], S[s]["month2"]), S[s]["month_wt1"], S[s]["month_wt2"] = pairs[s], 0.4, 0.6
    return S


# ---- timed regions ----

def back_to_back(D, fn, n):
    """ms per call of n calls of fn back to back, after one warm-up call."""
    fn()
    D.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    D.sync()
    return (time.perf_counter() - t0) / n * 1e3


def run_ms(D, steps, flags, n=3):
    """ms per step of elmk_run over `steps`, the snapshot restored before every run: one warm-up run, then n."""
    def once():
        D.restore_fields()
        D.run(DT, steps, flags)
    once()
    D.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        once()
    D.sync()
    return (time.perf_counter() - t0) / (n * len(steps)) * 1e3


def wall_ms(D, fn, sync_after=False):
    """Wall-clock ms of one call of fn on an idle device.  sync_after: for an fn that does not end in a call that waits."""
    D.sync()
    t0 = time.perf_counter()
    fn()
    if sync_after:
        D.sync()
    return (time.perf_counter() - t0) * 1e3


# ---- rounds ----

def interleave(r, keys):
    """The order of round r: the keys forward in even rounds, reversed in odd rounds."""
    keys = list(keys)
    return keys if r % 2 == 0 else keys[::-1]


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def medians(res):
    return {k: float(np.median(v)) for k, v in res.items()}


def spreads(res):
    return {k: spread(v) for k, v in res.items()}


# ---- this build beside other builds ----

def open_builds(cols, libs, build, first=None, optional=()):
    """libs: (key, path) pairs, path None for this build.  Loads the named builds, then creates one context per pair with
    build(cols, path) - the pair called `first` before the others - and returns {key: context} in the order of libs."""
    for _, p in libs:
        if p:
            load_build(p, optional)
    ctx = {}
    try:
        for k, p in sorted(libs, key=lambda kp: kp[0] != first):
            ctx[k] = build(cols, p)
    except BaseException:
        close_all(ctx)
        raise
    return {k: ctx[k] for k, _ in libs}


def close_all(ctx):
    for D in ctx.values():
        D.close()


def compare_libraries(cols, rounds, libs, build, time_one, first=None, optional=(), baseline=None, prepare=None):
    """Contexts of two or three builds in one process, taking turns: in every round each context gets one turn, in the order of libs in
    even rounds and reversed in odd rounds.  time_one(D) -> ms gives {"all": {key: [ms]}, "median", "spread"} and, with baseline,
    "<key>_over_<baseline>" of the medians for every other key.  A dict {mode: time_one} takes the modes in order inside every round,
    the contexts taking turns within each mode, and gives the three tables as {key: {mode: ...}}.  prepare({key: context}) runs once
    after the contexts exist.  All contexts are closed, in the order of libs."""
    ctx = open_builds(cols, libs, build, first, optional)
    try:
        if prepare:
            prepare(ctx)
        if callable(time_one):
            res = {k: [] for k in ctx}
            for r in range(rounds):
                for k in interleave(r, ctx):
                    res[k].append(time_one(ctx[k]))
            out = {"all": res, "median": medians(res), "spread": spreads(res)}
            for k in (ctx if baseline else ()):
                if k != baseline:
                    out[f"{k}_over_{baseline}"] = out["median"][k] / out["median"][baseline]
            return out
        res = {k: {m: [] for m in time_one} for k in ctx}
        for r in range(rounds):
            for m, fn in time_one.items():
                for k in interleave(r, ctx):
                    res[k][m].append(fn(ctx[k]))
        return {"all": res, "median": {k: medians(d) for k, d in res.items()}, "spread": {k: spreads(d) for k, d in res.items()}}
    finally:
        close_all(ctx)


# ---- command line ----

def arg(flag, **kw):
    return flag, kw


RUN_STEPS = arg("--run-steps", type=int, default=6)
AB = arg("--ab", default=None)
PARENT = arg("--parent", default=None)
PARENT_FIRST = arg("--parent-first", action="store_true")
PARENT2 = arg("--parent2", default=None)


def cli(cols, rounds, args=(), out=False):
    """--cols (a comma-separated list, parsed into a.cols) and --rounds with the tool's defaults, the tool's own arguments in their
    order, and --out for the tools that append their lines to a file."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default=cols)
    ap.add_argument("--rounds", type=int, default=rounds)
    for flag, kw in args:
        ap.add_argument(flag, **kw)
    if out:
        ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.cols = [int(c) for c in a.cols.split(",")]
    return a


def emit(record, out=None):
    """One JSON line on stdout, appended to the file `out` as well."""
    line = json.dumps(record)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def emit_each(a, one):
    """one(cols) -> a record or a list of records, for every column count of the command line."""
    for c in a.cols:
        r = one(c)
        for rec in (r if isinstance(r, list) else [r]):
            emit(rec, getattr(a, "out", None))
