"""Float64 restatement of the KL-divergence-to-queue loss (arco_amd/csrc/queue_kld.hip, stage1.queue_kld) and the inputs of its tests.
cs, ct: raw cosines [N, L]; s = cs / Ts, t = ct / Tt; the loss is F.kl_div(F.log_softmax(s, 1), F.softmax(t, 1), 'batchmean').
tests/test_queue_kld_cpu.py holds every function here to torch float64 autograd of that expression."""
import numpy as np

SHAPES = [(1, 1, 1), (3, 37, 37), (6, 36, 36), (5, 64, 64), (4, 257, 260), (2, 4099, 4099), (3, 70001, 70004)]      # (N, L, ld)
TEMPS = [(0.1, 0.1), (0.1, 0.01), (1.0, 0.07)]                                                                        # (Ts, Tt)


def _lse(x):
    m = x.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def stats(cs, ct, Ts, Tt):
    """[N, 3] float64: lse_s, lse_t, KL_i = sum_j p_ij ((t_ij - lse_t) - (s_ij - lse_s)) with p = softmax(t); p_ij == 0 adds 0."""
    s, t = np.asarray(cs, np.float64) / Ts, np.asarray(ct, np.float64) / Tt
    ls, lt = _lse(s), _lse(t)
    logp, logq = t - lt[:, None], s - ls[:, None]
    p = np.exp(logp)
    with np.errstate(invalid="ignore"):
        kl = np.where(p > 0, p * (logp - logq), 0.0).sum(axis=1)
    return np.stack([ls, lt, kl], axis=1)


def loss(cs, ct, Ts, Tt):
    return float(stats(cs, ct, Ts, Tt)[:, 2].sum() / np.asarray(cs).shape[0])


def grads(cs, ct, Ts, Tt, g=1.0):
    """(d loss / d cs, d loss / d ct) times the upstream gradient g:
    g (softmax(s) - p) / (N Ts)  and  g p ((t - lse_t) - (s - lse_s) - KL_i) / (N Tt)."""
    s, t = np.asarray(cs, np.float64) / Ts, np.asarray(ct, np.float64) / Tt
    st = stats(cs, ct, Ts, Tt)
    n = s.shape[0]
    logq, logp = s - st[:, 0:1], t - st[:, 1:2]
    p = np.exp(logp)
    with np.errstate(invalid="ignore"):
        inner = np.where(p > 0, p * (logp - logq - st[:, 2:3]), 0.0)
    return g * (np.exp(logq) - p) / (n * Ts), g * inner / (n * Tt)


def cosines(N, L, seed, dim=8):
    """Two [N, L] fp32 matrices of cosines between normalised `dim`-dimensional random vectors: they spread over the whole of [-1, 1]."""
    rs = np.random.RandomState(seed)

    def unit(n):
        v = rs.standard_normal((n, dim))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    q = unit(L)
    return (unit(N) @ q.T).astype(np.float32), (unit(N) @ q.T).astype(np.float32)


def hand_made(L, seed=0):
    """{name: (cs, ct, Ts, Tt)} - the rows that random cosines do not reach, each as a 2-row problem of length L."""
    rs = np.random.RandomState(1000 + seed)
    u = rs.uniform(-1, 1, (2, L)).astype(np.float32)
    v = rs.uniform(-1, 1, (2, L)).astype(np.float32)
    spike = np.full((2, L), -1.0, np.float32)
    spike[0, L // 3] = 1.0
    spike[1, L - 1] = 1.0
    low = (u * 0.5 - 0.5).astype(np.float32)           # in [-1, 0] ...
    low[0, L // 2] = 0.05                               # ... with the row maximum 0.05: a fixed shift by 1 / T = 100 underflows every term
    low[1, 0] = 0.05
    return {
        "equal": (u, u.copy(), 0.1, 0.1),
        "constant": (np.full((2, L), 0.25, np.float32), np.full((2, L), -0.5, np.float32), 0.1, 0.01),
        "spike": (u, spike, 0.01, 0.01),
        "spike_both": (spike, spike[::-1].copy(), 0.01, 0.01),
        "spike_f64": (u, spike, 0.1, 0.002),          # e^-1000: the other p are 0 in float64 as well (the kernels refuse nothing here either)
        "max_0p05": (v, low, 0.01, 0.01),
    }
