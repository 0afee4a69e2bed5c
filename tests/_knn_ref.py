"""References for distCUDA2 (pixie_amd/simple_knn.py), and the clouds the CPU and GPU tests share.

  brute32   chunked NumPy float32 brute force in the product's expression order: ((dx dx + dy dy) + dz dz) over all j != i (by
            index), the three smallest b0 <= b1 <= b2, ((b0 + b1) + b2) / 3; a missing neighbour is FLT_MAX.  NumPy does not fuse
            multiply-adds, so the product must equal it bit for bit.
  brute64   float64 on the same float32 coordinates: scipy.spatial.cKDTree, k = 4 (the point itself and three others).
TEST INFRASTRUCTURE ONLY."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def brute32(points, chunk=512):
    p = np.ascontiguousarray(points, np.float32)
    n = len(p)
    out = np.empty((n,), np.float32)
    with np.errstate(over="ignore"):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            d = p[None, :, :] - p[s:e, None, :]                      # q - p, float32
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d2[np.arange(e - s), np.arange(s, e)] = np.inf           # j != i by index
            if n < 4:
                d2 = np.concatenate([d2, np.full((e - s, 3), np.inf, np.float32)], axis=1)
            b = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
            b = np.where(np.isinf(b), FLT_MAX, b).astype(np.float32)
            out[s:e] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
    return out


def brute64(points):
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, np.float32).astype(np.float64)
    n = len(p)
    if n == 0:
        return np.empty((0,), np.float64)
    k = min(4, n)
    dist, _ = cKDTree(p).query(p, k=k)
    dist = dist.reshape(n, k)
    d2 = np.sort(dist, axis=1)[:, 1:] ** 2                           # the smallest is the point itself (0)
    if d2.shape[1] < 3:
        d2 = np.concatenate([d2, np.full((n, 3 - d2.shape[1]), float(FLT_MAX))], axis=1)
    return d2.sum(axis=1) / 3.0


def uniform(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)


def clustered(n=3000, seed=1):
    """half N(100, 1e-3), half N(0, 5): a tight far cluster beside a wide one"""
    rng = np.random.default_rng(seed)
    a = rng.normal(100.0, 1e-3, size=(n // 2, 3))
    b = rng.normal(0.0, 5.0, size=(n - n // 2, 3))
    return rng.permutation(np.concatenate([a, b])).astype(np.float32)


def planar(n=2000, seed=2):
    """z == 0: an axis of zero extent"""
    p = uniform(n, seed)
    p[:, 2] = 0.0
    return p


def coincident(n=100):
    return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (n, 1))


def collinear(n=300, seed=3):
    t = np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n, 1))
    return (t * np.array([[1.0, 2.0, -0.5]]) + np.array([[0.1, 0.2, 0.3]])).astype(np.float32)


def duplicated(n=500, seed=4):
    p = uniform(n, seed)
    return np.random.default_rng(seed + 1).permutation(np.concatenate([p, p]))


CLOUDS = {"clustered": clustered, "planar": planar, "coincident": coincident, "collinear": collinear, "duplicated": duplicated}
