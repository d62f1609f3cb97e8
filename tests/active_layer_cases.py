"""The soil columns of the active layer tests, host and device."""
import numpy as np

TFRZ = 273.15


def columns(n, seed, special=True):
    """t_soisno, zsoi [20, n]: random around tfrz over a monotone soil mesh; with `special`, hand-built columns first: every k from -1
    to 14, a talik, a layer at exactly tfrz, t1 - t2 of one ulp, NaN and infinities in t_soisno and zsoi."""
    rng = np.random.default_rng(seed)
    t = TFRZ + 3.0 * rng.standard_normal((20, n))
    z = np.cumsum(0.02 + rng.random((20, n)), axis=0) - 0.5
    if not special:
        return t, z
    c = 0

    def put(tt, zz=None):
        nonlocal c
        if c < n:
            t[5:, c] = tt
            if zz is not None:
                z[5:, c] = zz
        c += 1

    cold, warm = np.full(15, 271.15), 275.15
    for k in range(-1, 15):  # thawed down to layer k, frozen below
        tt = cold.copy()
        tt[:k + 1] = warm
        put(tt)
    tt = cold.copy()
    tt[14] = warm  # only the bottom layer thawed
    put(tt)
    tt = cold.copy()
    tt[[0, 1, 6, 7]] = warm  # a talik: thawed below frozen below thawed -> k = 7
    put(tt)
    tt = cold.copy()
    tt[:3] = warm
    tt[3] = TFRZ  # exactly tfrz is frozen -> k = 2, t2 = tfrz
    put(tt)
    tt = cold.copy()
    tt[:5] = TFRZ  # nothing above tfrz at all
    put(tt)
    tt = np.full(15, np.nextafter(TFRZ, 0.0))
    tt[4] = np.nextafter(TFRZ, 1e9)  # t1 - t2 = two ulps, t1 - tfrz = one ulp
    put(tt)
    tt = cold.copy()
    tt[5] = warm
    tt[6] = np.nextafter(warm, 0.0)  # t1 - t2 of one ulp, t[6] thawed: k = 6 against a frozen 7
    tt[4] = np.nextafter(warm, 1e9)
    put(tt)
    tt = np.full(15, warm)
    tt[9:] = np.nextafter(warm, 0.0)
    tt[14] = 271.15  # k = 13; above it t[k] - t[k+1] is large, but t[8] - t[9] = 1 ulp is never used
    put(tt)
    for bad in (np.nan, np.inf, -np.inf):
        for where in (14, 3, 0):
            tt = cold.copy()
            tt[:3] = warm
            tt[where] = bad
            put(tt)
        tt = cold.copy()
        tt[:4] = warm
        tt[4] = bad  # t2 is bad (k = 3), or +inf is thawed itself (k = 4)
        put(tt)
        for where in (2, 3, 14):
            tt = cold.copy()
            tt[:3] = warm
            zz = np.cumsum(np.full(15, 0.25))
            zz[where] = bad
            put(tt, zz)
        tt = np.full(15, warm)
        zz = np.cumsum(np.full(15, 0.25))
        zz[14] = bad  # the bottom layer thawed over a bad depth
        put(tt, zz)
    tt = cold.copy()
    tt[:2] = warm
    put(tt, np.zeros(15))  # z2 - z1 = 0
    return t, z
