"""Global conservation diagnostics across ranks.

The physics path has no exchange step; the one natural collective is the reduction of the conservation
diagnostics (elmk_evaluate_conservation returns (min, max, sum) over a rank's columns) to the whole domain: MIN, MAX
and SUM all-reduces of an [8, 3] array - 192 bytes, off the timed path.  This mirrors the reference's min_max_sum
over MPI (src/utils/min_max_sum.hh:57-66) with torch.distributed (RCCL on GPUs, gloo in the CPU tests)."""
import numpy as np


def local_min_max_sum(per_column):
    """[ncols, k] -> [k, 3] (min, max, sum), the host-side form of what the device reduction returns."""
    a = np.asarray(per_column, dtype=np.float64)
    return np.stack([a.min(axis=0), a.max(axis=0), a.sum(axis=0)], axis=1)


CONS_NPART, CONS_BLOCK = 512, 256  # ELMK_CONS_NPART workgroups of 256 threads (elmkernels_amd/csrc/k_surface_fluxes.hip)


def _sticky_min(a, b):
    """The device's select acc = (v < acc || v != v) ? v : acc: a NaN v is taken, and a NaN acc is only ever replaced by a NaN."""
    return np.where((b < a) | np.isnan(b), b, a)


def _sticky_max(a, b):
    return np.where((b > a) | np.isnan(b), b, a)


def _tree(mn, mx, sm):
    """The workgroup's tree over the last axis (256): s = 128, 64, .., 1: a[t] = op(a[t], a[t + s]) for t < s."""
    s = mn.shape[-1] // 2
    while s:
        mn = _sticky_min(mn[..., :s], mn[..., s:2 * s])
        mx = _sticky_max(mx[..., :s], mx[..., s:2 * s])
        sm = sm[..., :s] + sm[..., s:2 * s]
        s //= 2
    return mn[..., 0], mx[..., 0], sm[..., 0]


def reduce_min_max_sum(x):
    """(min, max, sum) of the values x [n] in the device reduction's order, bit for bit (k_cons_reduce1 / k_cons_reduce2 /
    k_cons_reduce2_run): what elmk_evaluate_conservation and a row of elmk_run_diagnostics hold for one diagnostic.

    Stage 1: T = 512 x 256 threads; thread g folds x[g], x[g + T], x[g + 2T], .. in that order into (+inf, -inf, +0.0); every
    workgroup of 256 consecutive threads then tree-reduces (s = 128 .. 1: a[t] = op(a[t], a[t + s])) to one partial triple.
    Stage 2: thread j of one workgroup folds partials j, j + 256 from the same identity; the same tree follows.
    min / max are NaN-sticky (a NaN anywhere gives NaN; of +0.0 and -0.0 the one met first stays), the sum is the plain fp64 sum.
    Padding x to whole trips with +0.0 (sum) and the identities (min, max) changes no bit: an accumulator that starts at +0.0 is never
    -0.0 (only -0.0 + -0.0 rounds to -0.0), and s + (+0.0) == s bitwise for every s that is not -0.0."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    T = CONS_NPART * CONS_BLOCK
    trips = max(1, -(-x.size // T))
    pad = trips * T - x.size

    def padded(fill):
        return np.concatenate([x, np.full(pad, fill)]).reshape(trips, CONS_NPART, CONS_BLOCK)

    vmin, vmax, vsum = padded(np.inf), padded(-np.inf), padded(0.0)
    mn = np.full((CONS_NPART, CONS_BLOCK), np.inf)
    mx = np.full((CONS_NPART, CONS_BLOCK), -np.inf)
    sm = np.zeros((CONS_NPART, CONS_BLOCK))
    with np.errstate(invalid="ignore"):  # (+inf) + (-inf), comparisons with NaN
        for t in range(trips):
            mn, mx, sm = _sticky_min(mn, vmin[t]), _sticky_max(mx, vmax[t]), sm + vsum[t]
        pmn, pmx, psm = _tree(mn, mx, sm)  # [512] partials
        mn, mx, sm = np.full(CONS_BLOCK, np.inf), np.full(CONS_BLOCK, -np.inf), np.zeros(CONS_BLOCK)
        for r in range(CONS_NPART // CONS_BLOCK):
            sl = slice(r * CONS_BLOCK, (r + 1) * CONS_BLOCK)
            mn, mx, sm = _sticky_min(mn, pmn[sl]), _sticky_max(mx, pmx[sl]), sm + psm[sl]
        mn, mx, sm = _tree(mn, mx, sm)
    return np.array([mn, mx, sm])


def global_min_max_sum(mms, group=None, device=None):
    """All-reduce a rank-local [k, 3] (min, max, sum) array over the process group -> the global one on every rank."""
    import torch
    import torch.distributed as dist

    mms = np.ascontiguousarray(mms, dtype=np.float64)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return mms.copy()
    t = torch.from_numpy(mms.copy())
    if device is not None:
        t = t.to(device)
    mn, mx, sm = t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous()
    dist.all_reduce(mn, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
    dist.all_reduce(sm, op=dist.ReduceOp.SUM, group=group)
    return torch.stack([mn, mx, sm], dim=1).cpu().numpy()
