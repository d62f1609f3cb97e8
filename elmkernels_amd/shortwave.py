"""Shortwave COSZEN mode on the host (include/elmk.h "shortwave"): ELM's cos(zenith) factor that spreads an interval-mean FSDS record
over the model steps of its interval.  numpy only; the device applies the same operation in ProcessFSDS (k_forcing.hip)."""
import numpy as np

SW_REFERENCE, SW_COSZEN = 0, 1  # elmk_set_shortwave_mode
SW_MODES = {"reference": SW_REFERENCE, "coszen": SW_COSZEN}


def coszen_factor(cz, czf):
    """fac = (cz > 0.001) ? min(cz / czf, 10.0) : 0.0 elementwise, min as std::min (the first argument wins ties and NaN).

    Written with explicit comparisons: np.minimum returns NaN for a NaN in either argument, std::min(a, b) = (b < a) ? b : a
    returns a whenever the comparison is false."""
    cz = np.asarray(cz, dtype=np.float64)
    czf = np.asarray(czf, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = cz / czf
    capped = np.where(10.0 < q, 10.0, q)
    return np.where(cz > 0.001, capped, 0.0)
