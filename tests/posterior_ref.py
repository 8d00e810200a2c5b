"""The numpy float64 reference of the posterior-aware scores: the bf16 image of tanh(dec-0) of S samples of z per user, the
decoder product reduced over the samples to mean / std / score, the one derived tolerance, and the fixture the CPU and GPU tests share.
Pure numpy: no GPU, no package import."""
import numpy as np

H, Z, K_PAD = 600, 200, 608
SAMPLES = (1, 4, 8, 16, 32)
STREAM_POSTERIOR_EPS = 9


def bf16_round(x):
    """float -> the nearest bf16 (ties to even), as float32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits_to_float(bits):
    """the int16 / uint16 words of a device image -> their values as float32"""
    return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def sample_z(mulv, eps):
    """mulv [n, 2Z] (mu | logvar), eps [n, S, Z] -> z [n, S, Z] float64 = mu + exp(logvar / 2) * eps"""
    mulv, eps = np.asarray(mulv, np.float64), np.asarray(eps, np.float64)
    zd = mulv.shape[1] // 2
    return mulv[:, None, :zd] + np.exp(0.5 * mulv[:, None, zd:]) * eps


def h2_image(mulv, eps, W_p0, b_p0):
    """-> (image [n * S, H] float32 holding bf16 values, h [n * S, H] float64 before the rounding, z [n * S, Z] float64);
    row r * S + s = sample s of user r"""
    z = sample_z(mulv, eps)
    z = z.reshape(-1, z.shape[2])
    h = np.tanh(z @ np.asarray(W_p0, np.float64) + np.asarray(b_p0, np.float64))
    return bf16_round(h.astype(np.float32)), h, z


def sample_logits(image, W_bf16, b, S):
    """image [n * S, K] and W_bf16 [I, K] (bf16 values as floats), b [I] -> l [n, S, I] float64"""
    image, W = np.asarray(image, np.float64), np.asarray(W_bf16, np.float64)
    return (image @ W.T + np.asarray(b, np.float64)).reshape(-1, S, W.shape[0])


def scores(image, W_bf16, b, S, beta):
    """-> (score, mean, std), each [n, I] float64: the mean and the POPULATION std over the S samples, score = mean + beta * std"""
    l = sample_logits(image, W_bf16, b, S)
    mean = l.mean(1)
    std = np.sqrt(((l - mean[:, None, :]) ** 2).mean(1))
    return mean + beta * std, mean, std


def brute_scores(image, W_bf16, b, S, beta):
    """the definition, one (user, item, sample) at a time -- slow, for tiny shapes"""
    image, W, b = np.asarray(image, np.float64), np.asarray(W_bf16, np.float64), np.asarray(b, np.float64)
    n, I = image.shape[0] // S, W.shape[0]
    out = np.zeros((3, n, I))
    for r in range(n):
        for i in range(I):
            ls = [float(np.dot(image[r * S + s], W[i])) + float(b[i]) for s in range(S)]
            m = sum(ls) / S
            sd = (sum((x - m) ** 2 for x in ls) / S) ** 0.5
            out[:, r, i] = (m + beta * sd, m, sd)
    return out[0], out[1], out[2]


def magnitude(image, W_bf16, b, S):
    """A [n, I] = max over the samples of sum_k |h_k| |w_k| + |b|: what an fp32 accumulation's error scales with"""
    a = np.abs(np.asarray(image, np.float64)) @ np.abs(np.asarray(W_bf16, np.float64)).T + np.abs(np.asarray(b, np.float64))
    return a.reshape(-1, S, a.shape[1]).max(1)


def bound(image, W_bf16, b, S, K=K_PAD):
    """The one tolerance, per element [n, I], derived and not measured: fp32 accumulation over K terms is off by at most K 2^-24 A per
    sample; the mean adds S 2^-24 max|l| <= S 2^-24 A; the two-pass std is 1-Lipschitz in the largest per-sample error; bias add and
    final roundings are the + 2.  tol = 2 (K + S + 2) 2^-24 A for mean, std and (beta = 0) score alike, the 2 being the safety margin.
    A score at |beta| <= 2 gets 3 tol."""
    return 2.0 * (K + S + 2) * 2.0 ** -24 * magnitude(image, W_bf16, b, S)


def xavier(rng, fan_in, fan_out, shape):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def fixture(n, I, S, seed=20261):
    """The shared fixture: H = 600, Z = 200, Xavier weights in engine layout, biases N(0, 1e-3), mu ~ N(0, 1), logvar ~ U(-2, 0),
    eps ~ N(0, 1) -> dict of float32 arrays (gen: the eight generator arrays as Engine.set_generator takes them)"""
    rng = np.random.default_rng(seed)
    gen = [xavier(rng, I, H, (I, H)), xavier(rng, H, 2 * Z, (H, 2 * Z)), xavier(rng, Z, H, (Z, H)), xavier(rng, H, I, (I, H)),
           (1e-3 * rng.standard_normal(H)).astype(np.float32), (1e-3 * rng.standard_normal(2 * Z)).astype(np.float32),
           (1e-3 * rng.standard_normal(H)).astype(np.float32), (1e-3 * rng.standard_normal(I)).astype(np.float32)]
    mulv = np.concatenate([rng.standard_normal((n, Z)), rng.uniform(-2.0, 0.0, (n, Z))], 1).astype(np.float32)
    eps = rng.standard_normal((n, S, Z)).astype(np.float32)
    return dict(gen=gen, W_p0=gen[2], b_p0=gen[6], W_p1t=gen[3], b_p1=gen[7], W_bf16=bf16_round(gen[3]), mulv=mulv, eps=eps, n=n, I=I, S=S)


def pad_k(a, K=K_PAD):
    """[rows, H] -> [rows, K] with zero columns"""
    out = np.zeros((a.shape[0], K), a.dtype)
    out[:, : a.shape[1]] = a
    return out
