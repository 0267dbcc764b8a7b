"""The node sets and table contents that the CPU and the GPU tests of a 2-D table set installed from device memory share
(test_tabulated_install_host.py, test_gpu_tabulated_install.py).  Test infrastructure only."""
import numpy as np

GLO, GHI = 1.01, 1e4        # the range of a set on nodes uniform in ln gamma


def graded_gamma(n, rng):
    """n gamma nodes whose steps in ln gamma are spread log-uniformly over six decades, the widest and the narrowest side by
    side, from ln gamma = 0.01 over a range of 9 (gamma to 8e3)"""
    h = 10.0 ** rng.uniform(-6.0, 0.0, n - 1)
    h[0], h[1] = h.max(), h.max() * 1e-6
    u = 0.01 + np.concatenate([[0.0], np.cumsum(h * (9.0 / h.sum()))])
    g = np.exp(u)
    assert (np.diff(np.log(g)) > 0).all() and g[0] >= 1.0
    return g


def graded_mu(n, rng):
    """n mu nodes from exactly -1 to exactly +1 whose cell widths are spread log-uniformly over four decades, the widest and
    the narrowest side by side"""
    w = 10.0 ** rng.uniform(-4.0, 0.0, n - 1)
    w[-2], w[-1] = w.max(), w.max() * 1e-4
    m = -1.0 + np.concatenate([[0.0], np.cumsum(w * (2.0 / w.sum()))])
    m[0], m[-1] = -1.0, 1.0
    assert (np.diff(m) > 0).all()
    return m


def nodes_of(form, shape, rng):
    """(gamma, mu) as the entry of `form` takes them -- None where the form places its own nodes -- and (gamma, mu) where the
    nodes lie.  form: "uniform", "grid" (given gamma nodes) or "nodes" (given gamma and mu nodes)."""
    nt, nn, nmu = shape
    if form == "uniform":
        return None, None, np.exp(np.linspace(np.log(GLO), np.log(GHI), nn)), np.linspace(-1.0, 1.0, nmu)
    gamma = graded_gamma(nn, rng)
    if form == "grid":
        return gamma, None, gamma, np.linspace(-1.0, 1.0, nmu)
    mu = graded_mu(nmu, rng)
    return gamma, mu, gamma, mu


def smooth(shape, gamma, mu, rng, jitter=0.02):
    """ln n of a power law per table, rolled off at both ends of the nodes and tilted in mu more the higher gamma, each value
    moved by a seeded +-2 % (jitter = 0: the surface itself, which every form's normalisation integrates to a number)"""
    nt = shape[0]
    u, g, m = np.log(gamma)[None, :, None], gamma[None, :, None], mu[None, None, :]
    p = (2.0 + 0.5 * np.arange(nt))[:, None, None]
    t = -p * u + 0.05 * u * m + 0.7 * m - 2.0 / g - 5.0 * g / gamma[-1]
    return np.ascontiguousarray(t * (1.0 + rng.uniform(-jitter, jitter, shape)))


def rough(shape, rng):
    """values all over +-700, no two neighbours alike"""
    return rng.uniform(-700.0, 700.0, shape)
