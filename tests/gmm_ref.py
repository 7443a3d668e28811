"""float64 numpy restatement of include/svae_gmm.h (helper of the mixture tests, not collected): the E part with its dimension
and component loops in index order, the centred M part, the freeze rule of svae_gmm_step and ops.GaussianMixture.fit.  Every
sum over points is kmeans_ref's two-level one.  Adding +0 for a point that does not take part is exact, so masked values stand
for skipped ones.  `fn` carries exp and log, so that a test can perturb them (Ulps)."""
import numpy as np

import kmeans_ref as K

LOG_2PI = float(np.log(2.0 * np.pi))


class Exact(object):
    exp, log = staticmethod(np.exp), staticmethod(np.log)


class Ulps(object):
    """exp and log with every result moved by a random whole number of ulps in [-n, n]."""

    def __init__(self, seed, n=4):
        self.rs, self.n = np.random.RandomState(seed), n

    def _move(self, v):
        v = np.asarray(v, np.float64)
        step = self.rs.randint(-self.n, self.n + 1, size=v.shape)
        return np.where(np.isfinite(v) & (v != 0), v + step * np.spacing(v), v)

    def exp(self, v):
        return self._move(np.exp(v))

    def log(self, v):
        return self._move(np.log(v))


def scores(x, weight, mean, var, fn=Exact):
    """a (N, k) of the header: -inf in the column of a dead component; rows of non-finite points hold nothing meaningful."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    N, D = x64.shape
    k = weight.shape[0]
    a = np.full((N, k), -np.inf)
    with np.errstate(all="ignore"):
        for j in np.nonzero(weight > 0)[0]:
            iv = 1.0 / var[j]
            lv = np.cumsum(fn.log(var[j]))[-1] + 0.0
            c = fn.log(weight[j]) - 0.5 * (lv + float(D) * LOG_2PI)
            q = np.zeros(N)
            for t in range(D):
                d = x64[:, t] - mean[j, t]
                q += (d * d) * iv[t]
            a[:, j] = c - 0.5 * q
    return a


def e_part(x, weight, mean, var, fn=Exact):
    """{resp (N, k), label (N) int64, loglik_point (N), loglik, assigned, a}."""
    a = scores(x, weight, mean, var, fn)
    N, k = a.shape
    m, label = np.full(N, -np.inf), np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for j in range(k):
            better = a[:, j] > m
            m[better], label[better] = a[better, j], j
        ok = K.finite_rows(x) & (m > -np.inf)
        e = np.zeros((N, k))
        s = np.zeros(N)
        for j in range(k):
            e[ok, j] = fn.exp(a[ok, j] - m[ok])
            s[ok] += e[ok, j]
        resp = np.zeros((N, k))
        resp[ok] = e[ok] / s[ok, None]
        ll = np.zeros(N)
        ll[ok] = m[ok] + fn.log(s[ok])
    label[~ok] = -1
    return {"resp": resp, "label": label, "loglik_point": ll, "loglik": float(K.ordered_sum(ll)), "assigned": int(ok.sum()), "a": a}


def m_part(x, resp, weight, mean, var, reg, assigned):
    """(weight, mean, var) after the M part about the incoming mean; a component with !(R > 0) gets weight 0 and keeps the rest."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = x64[:, None, :] - mean[None]
    d[~K.finite_rows(x)] = 0.0                       # their resp rows are all zero: + 0
    R = K.ordered_sum(resp)
    S1 = K.ordered_sum(resp[:, :, None] * d)
    S2 = K.ordered_sum(resp[:, :, None] * (d * d))
    weight, mean, var = np.zeros_like(weight), mean.copy(), var.copy()
    live = R > 0
    delta = S1[live] / R[live, None]
    mean[live] = mean[live] + delta
    var[live] = np.maximum(S2[live] / R[live, None] - delta * delta, 0.0) + reg
    weight[live] = R[live] / float(assigned)
    return weight, mean, var


def init(x, label_in, centres, reg):
    """svae_gmm_init: the state dict {weight, mean, var, resp, iterations, converged_at, assigned, dead, loglik, previous}."""
    x = np.asarray(x, np.float32)
    centres = np.asarray(centres, np.float64)
    k = centres.shape[0]
    label_in = np.asarray(label_in)
    fin = K.finite_rows(x)
    resp = ((label_in[:, None] == np.arange(k)[None]) & fin[:, None]).astype(np.float64)
    assigned = int(fin.sum())
    weight, mean, var = m_part(x, resp, np.zeros(k), centres, np.zeros_like(centres), reg, assigned)
    return {"weight": weight, "mean": mean, "var": var, "resp": resp, "iterations": 0, "converged_at": 0, "assigned": assigned,
            "dead": int((~(weight > 0)).sum()), "loglik": 0.0, "previous": 0.0}


def step(x, state, update, reg, tol, fn=Exact):
    """One svae_gmm_step on a state dict; returns the new one, with label, loglik_point, a and `gain` (loglik - previous where
    the rule looked at it, else None) added."""
    e = e_part(x, state["weight"], state["mean"], state["var"], fn)
    out = dict(state, resp=e["resp"], label=e["label"], loglik_point=e["loglik_point"], loglik=e["loglik"], assigned=e["assigned"],
               a=e["a"], gain=None)
    if update and state["converged_at"] == 0:
        L = e["loglik"]
        if state["iterations"] >= 1:
            out["gain"] = L - state["previous"]
        if state["iterations"] >= 1 and L - state["previous"] <= tol * abs(L):
            out["converged_at"] = state["iterations"]
        else:
            out["weight"], out["mean"], out["var"] = m_part(x, e["resp"], state["weight"], state["mean"], state["var"], reg, e["assigned"])
            out["iterations"] = state["iterations"] + 1
            out["previous"] = L
    out["dead"] = int((~(out["weight"] > 0)).sum())
    return out


def fit(x, label_in, centres, iters, reg, tol, fn=Exact):
    """ops.GaussianMixture.fit: init, `iters` update steps, one labelling step.  The last state with trace (iters + 1) and gains
    (the deciding gains of the update steps, None where the rule did not look) added."""
    state = init(x, label_in, centres, reg)
    trace, gains = [], []
    for update in [1] * iters + [0]:
        state = step(x, state, update, reg, tol, fn)
        trace.append(state["loglik"])
        if update:
            gains.append(state["gain"])
    return dict(state, trace=np.array(trace), gains=gains)


def top_two_gap(a):
    """The smallest gap between the best and the second-best score of a row of a (N, k), over rows with a finite best."""
    if a.shape[1] < 2:
        return np.inf
    order = np.sort(a, 1)
    rows = np.isfinite(order[:, -1])
    return float((order[rows, -1] - order[rows, -2]).min())


def planted(seed, N, D, k):
    """kmeans_ref.blobs again with what it keeps to itself: (x, planted label, planted centres); x is blobs' x bit for bit."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(min(k, 6), D) * 2
    label = rs.randint(0, centres.shape[0], size=N)
    return (centres[label] + 0.35 * rs.randn(N, D)).astype(np.float32), label, centres


# The fixtures of the kernel tests: (seed, N, D, k, spread of the planted centres; 0.35 is the noise, so 0.6 overlaps).
FIXTURES = [(0, 300, 3, 4, 2.0), (1, 257, 1, 2, 2.0), (2, 1000, 8, 6, 0.6), (3, 700, 5, 10, 0.6), (4, 513, 64, 3, 2.0),
            (5, 600, 64, 32, 2.0), (6, 900, 8, 40, 2.0), (7, 262145, 2, 2, 2.0),
            (8, 300, 4, 3, 2.0), (9, 300, 16, 3, 2.0), (10, 300, 17, 3, 2.0)]     # D on the 4 / 16 / 64 register bounds
FIT_STEPS, FIT_REG, FIT_TOL = 25, 1e-6, 1e-6
_cache = {}


def fixture(seed, N, D, k, spread):
    """(x, label_in, centres): k planted centres randn * spread, noise 0.35 randn, fp32; the start is 5 steps of kmeans_ref.fit
    from the uniforms RandomState(100 + seed).rand(k).  Computed once per process."""
    key = ("fixture", seed, N, D, k, spread)
    if key not in _cache:
        rs = np.random.RandomState(seed)
        centres = rs.randn(k, D) * spread
        x = (centres[rs.randint(0, k, size=N)] + 0.35 * rs.randn(N, D)).astype(np.float32)
        km = K.fit(x, k, np.random.RandomState(100 + seed).rand(k), 5)
        _cache[key] = (x, km["label"].astype(np.int32), km["centres"])
    return _cache[key]


def fixture_states(seed, N, D, k, spread):
    """The reference's states along the fixture's fit: [init, after each of FIT_STEPS update steps, after the labelling step].
    Computed once per process and never changed."""
    key = ("states", seed, N, D, k, spread)
    if key not in _cache:
        x, label_in, centres = fixture(seed, N, D, k, spread)
        states = [init(x, label_in, centres, FIT_REG)]
        for update in [1] * FIT_STEPS + [0]:
            states.append(step(x, states[-1], update, FIT_REG, FIT_TOL))
        _cache[key] = states
    return _cache[key]
