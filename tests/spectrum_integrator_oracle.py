"""Oracle of the spectrum integrator (include/gr4hip.h, gr4hip_specint_*; SPECTRUM_INTEGRATOR.md).  The reference has no such block, so this file IS the definition:
frames m[f][c]; output q covers frames [q A, (q + 1) A), leaf l of it frames q A + [32 l, min(32 (l + 1), A));

    leaf_l[c] = (((0 + m[f0][c]) + m[f0 + 1][c]) + ...)              float32, frames ascending
    acc[c]    = ((0 + (double)leaf_0[c]) + (double)leaf_1[c]) + ...  float64, leaves ascending
    y_q[c]    = (float)acc[c]   or, mean,   (float)(acc[c] / (double)A)

integrate is the plain float64 sum, integrate_ordered the definition with numpy float32 / float64 arithmetic (IEEE, element-wise, in the stated order).  A trailing
incomplete integration is dropped by both."""
import numpy as np

LEAF = 32


def signal(n, seed):
    """the tests' signal: unit complex noise plus a tone of amplitude 4 at 0.2137 fs"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + 4.0 * np.exp(2j * np.pi * 0.2137 * np.arange(n))
    return x.astype(np.complex64)


def integrate(m, A, mean=False):
    """float64 [frames // A, N]"""
    m = np.asarray(m, np.float64)
    q = m.shape[0] // A
    y = m[:q * A].reshape(q, A, m.shape[1]).sum(axis=1)
    return y / A if mean else y


def integrate_ordered(m, A, mean=False):
    """float32 [frames // A, N], the definition's additions one by one"""
    m = np.asarray(m, np.float32)
    q, N = m.shape[0] // A, m.shape[1]
    y = np.empty((q, N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q):
            acc = np.zeros(N, np.float64)
            for s in range(0, A, LEAF):
                leaf = np.zeros(N, np.float32)
                for f in range(i * A + s, i * A + min(s + LEAF, A)):
                    leaf = leaf + m[f]  # float32 + float32 -> one IEEE float32 add
                acc = acc + leaf.astype(np.float64)
            y[i] = (acc / np.float64(A) if mean else acc).astype(np.float32)
    return y
