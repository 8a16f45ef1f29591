"""A plain numpy fp64 restatement of the exact t-SNE contracts of csrc/tsne.hip and sm3hip/tsne.py, shared by
tests/test_tsne_cpu.py, tests/test_tsne_gpu.py and tests/golden/gen_tsne_golden.py.  No early exit anywhere; every sum that the
kernels take in "the fixed order" goes through fixed_sum."""
import numpy as np

STEPS = 100          # bisection steps of the precision search, always all of them
MIN_GAIN = 0.01
MAX_POINTS = 16384


def blobs(N=300, D=16, k=6, seed=0):
    """k Gaussian islands: centres 4 * randn, point n = centre[n % k] + randn, one RandomState(seed); ([N, D] float32, labels)."""
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.randn(k, D)
    labels = np.arange(N) % k
    return (centres[labels] + rs.randn(N, D)).astype(np.float32), labels


def fixed_sum(t):
    """The sum over the last axis in the kernels' order: partial t adds the terms j = t, t + 256, ... in ascending j, then the 256
    partials fold by the halving tree a[t] += a[t + h], h = 128, 64 .. 1.  A function of the terms and their number alone."""
    t = np.asarray(t, dtype=np.float64)
    n = t.shape[-1]
    k = max(1, -(-n // 256))
    pad = np.zeros(t.shape[:-1] + (k * 256,), dtype=np.float64)
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (k, 256))
    a = pad[..., 0, :].copy()
    for c in range(1, k):
        a = a + pad[..., c, :]
    h = 128
    while h:
        a = a[..., :h] + a[..., h:2 * h]
        h >>= 1
    return a[..., 0]


def sqdist(x):
    """D2[i, j] = sum_k (x_ik - x_jk)^2 in fp64, the diagonal 0."""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    d2 = np.einsum("ijk,ijk->ij", d, d)
    np.fill_diagonal(d2, 0.0)
    return d2


def _shifted(d2):
    d2 = np.asarray(d2, dtype=np.float64)
    N = d2.shape[0]
    eye = np.eye(N, dtype=bool)
    m = np.where(eye, np.inf, d2).min(axis=1)
    dp = d2 - m[:, None]
    dp[eye] = 0.0  # not a term of any sum
    return dp, eye


def row_entropy(d2, beta):
    """H_i(beta_i) = log S0 + beta S1 / S0 of the shifted row, S0 = sum_j e_j, S1 = sum_j d'_j e_j, e_j = exp(-(beta d'_j))."""
    dp, eye = _shifted(d2)
    beta = np.asarray(beta, dtype=np.float64)
    e = np.exp(-(beta[:, None] * dp))
    e[eye] = 0.0
    S0, S1 = fixed_sum(e), fixed_sum(dp * e)
    return np.log(S0) + beta * S1 / S0, e, S0


def conditional(d2, perplexity, steps=STEPS):
    """(c [N, N] fp64 with c_ii = 0, beta [N]): scikit-learn's _binary_search_perplexity on the row minus its least off-diagonal
    entry, `steps` steps without a tolerance, then the row at the last beta."""
    N = np.asarray(d2).shape[0]
    target = np.log(np.float64(perplexity))
    beta, lo, hi = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    for _ in range(steps):
        H, _, _ = row_entropy(d2, beta)
        up = H > target
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        with np.errstate(invalid="ignore", over="ignore"):
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0),
                            np.where(np.isinf(lo), beta / 2.0, (beta + lo) / 2.0))
    _, e, S0 = row_entropy(d2, beta)
    return e / S0[:, None], beta


def row_perplexity(c):
    """exp(-sum_j c_ij log c_ij) of every row (0 log 0 = 0)."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(c > 0, c * np.log(c), 0.0)
    return np.exp(-t.sum(axis=1))


def symmetrise(c32):
    """P = fp32((double(c_ij) + double(c_ji)) / (2 N))."""
    c = np.asarray(c32, dtype=np.float32).astype(np.float64)
    return ((c + c.T) / np.float64(2 * c.shape[0])).astype(np.float32)


def pair_weights(y32, arithmetic="fp64"):
    """(w, dx, dy) [N, N] fp64 of the fp32 map y32.  "fp64": exact differences and w in fp64 (the restatement).  "fp32": the
    kernel's pair arithmetic -- dx, dy, q = fma(dy, dy, fma(dx, dx, 1)) and w = 1 / q each rounded to fp32 -- then widened."""
    y = np.asarray(y32, dtype=np.float32)
    if arithmetic == "fp32":
        dx = (y[:, None, 0] - y[None, :, 0]).astype(np.float32)
        dy = (y[:, None, 1] - y[None, :, 1]).astype(np.float32)
        q = (dx.astype(np.float64) ** 2 + 1.0).astype(np.float32)          # an fp32 square is exact in fp64: one rounding each
        q = (dy.astype(np.float64) ** 2 + q.astype(np.float64)).astype(np.float32)
        w = (np.float32(1.0) / q).astype(np.float64)
        return w, dx.astype(np.float64), dy.astype(np.float64)
    y = y.astype(np.float64)
    dx = y[:, None, 0] - y[None, :, 0]
    dy = y[:, None, 1] - y[None, :, 1]
    return 1.0 / (1.0 + dx * dx + dy * dy), dx, dy


def forces(P, y32, arithmetic="fp64", absolute=False):
    """F [N, 5] fp64 = (Z_i, A_i.x, A_i.y, R_i.x, R_i.y) over j != i in the fixed order; absolute: the sums of the terms'
    absolute values instead (what the error bound of the test scales with)."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    w, dx, dy = pair_weights(y32, arithmetic)
    np.fill_diagonal(w, 0.0)
    terms = [w, P * w * dx, P * w * dy, w * w * dx, w * w * dy]
    if absolute:
        terms = [np.abs(t) for t in terms]
    return np.stack([fixed_sum(t) for t in terms], axis=1)


def update(F, exaggeration, momentum, lr, y32, upd32, gains32):
    """One step of scikit-learn's _gradient_descent from the force sums: (y, update, gains as fp32 [N, 2], g [N, 2] fp64,
    sum (gains g)^2, Z).  Everything in fp64 from the stored fp32 state, rounded once on store."""
    F = np.asarray(F, dtype=np.float64)
    Z = fixed_sum(F[:, 0])
    g = 4.0 * (np.float64(exaggeration) * F[:, 1:3] - F[:, 3:5] / Z)
    u = np.asarray(upd32, dtype=np.float32).astype(np.float64)
    gains = np.asarray(gains32, dtype=np.float32).astype(np.float64)
    gains = np.maximum(np.where(u * g < 0.0, gains + 0.2, gains * 0.8), MIN_GAIN)
    gg = gains * g
    u = np.float64(momentum) * u - np.float64(lr) * gg
    y = np.asarray(y32, dtype=np.float32).astype(np.float64) + u
    gn2 = fixed_sum(gg[:, 0] * gg[:, 0] + gg[:, 1] * gg[:, 1])
    return y.astype(np.float32), u.astype(np.float32), gains.astype(np.float32), g, float(gn2), float(Z)


def kl(P, y32, F, arithmetic="fp64"):
    """sum_{p_ij > 0} p_ij ((log p_ij - log w_ij) + log Z): row sums in the fixed order, then the rows in the fixed order."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    w, _, _ = pair_weights(y32, arithmetic)
    logZ = np.log(fixed_sum(np.asarray(F, dtype=np.float64)[:, 0]))
    pos = P > 0
    np.fill_diagonal(pos, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(pos, P * ((np.log(P) - np.log(w)) + logZ), 0.0)
    return float(fixed_sum(fixed_sum(t)))


def random_init(N, seed):
    import torch
    return (1e-4 * torch.randn(N, 2, generator=torch.Generator().manual_seed(seed))).numpy().astype(np.float32)


def learning_rate(N, exaggeration):
    return max(N / exaggeration / 4.0, 50.0)


def tsne(x, perplexity=30.0, iters=1000, exaggeration=12.0, exaggeration_iters=250, seed=0, check_every=50, min_grad_norm=1e-7,
         patience=300, arithmetic="fp64"):
    """The whole map by the schedule of sm3hip.tsne.tsne (init="random", learning_rate="auto"): {"map", "kl", "history",
    "iters_run", "beta", "P"}."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[0]
    c, beta = conditional(sqdist(x), perplexity)
    P = symmetrise(c.astype(np.float32))
    y = random_init(N, seed)
    upd, gains = np.zeros((N, 2), np.float32), np.ones((N, 2), np.float32)
    lr = learning_rate(N, exaggeration)
    history, best, best_it, it = [], np.inf, exaggeration_iters, 0
    for it in range(iters):
        early = it < exaggeration_iters
        F = forces(P, y, arithmetic)
        check = (it + 1) % check_every == 0
        if check:
            err = kl(P, y, F, arithmetic)
        y, upd, gains, _, gn2, _ = update(F, exaggeration if early else 1.0, 0.5 if early else 0.8, lr, y, upd, gains)
        if check:
            history.append((it, err, float(np.sqrt(gn2))))
            if not early:
                if err < best:
                    best, best_it = err, it
                elif it - best_it > patience:
                    break
                if np.sqrt(gn2) <= min_grad_norm:
                    break
    return {"map": y, "kl": kl(P, y, forces(P, y, arithmetic), arithmetic), "history": history, "iters_run": it + 1, "beta": beta,
            "P": P}


def trustworthiness(x, y, k=10):
    """scikit-learn's trustworthiness(X, Y, n_neighbors=k) with Euclidean distances (ties by the lower index)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    dx = sqdist(x)
    np.fill_diagonal(dx, np.inf)
    order_x = np.argsort(dx, axis=1, kind="stable")
    dy = sqdist(y)
    np.fill_diagonal(dy, np.inf)
    nn_y = np.argsort(dy, axis=1, kind="stable")[:, :k]
    rank = np.zeros((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order_x] = np.arange(1, n + 1)[None, :]
    r = rank[np.arange(n)[:, None], nn_y] - k
    t = float(r[r > 0].sum())
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
