"""The place-recognition definition (docs/kernels/place.md) as a numpy model: polar max-height descriptor, ring key, column
norms, shift-minimised column-cosine distance, ring-key prefilter and top-k.  Every f32 step is a numpy f32 op and every sum
runs in the stated order, so the device result equals this model bit for bit except for the f64 square root and division."""
import numpy as np

DEFAULTS = dict(n_ring=20, n_sector=60, min_range=0.3, max_range=80.0, height_offset=2.0)


class Config:
    def __init__(self, n_ring=20, n_sector=60, min_range=0.3, max_range=80.0, height_offset=2.0):
        self.n_ring, self.n_sector = int(n_ring), int(n_sector)
        self.min_range, self.max_range, self.height_offset = float(min_range), float(max_range), float(height_offset)
        k = np.arange(self.n_ring + 1, dtype=np.float64)
        self.e2 = ((k * self.max_range / self.n_ring) ** 2).astype(np.float32)
        self.lo2 = np.float32(self.min_range ** 2)
        h = np.arange(self.n_sector // 2, dtype=np.float64)
        self.bc = np.cos(2.0 * np.pi * h / self.n_sector).astype(np.float32)
        self.bs = np.sin(2.0 * np.pi * h / self.n_sector).astype(np.float32)


def bins(cfg, pts):
    """(ring, sector, v, keep) of every point; all f32."""
    p = np.asarray(pts, np.float32).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r2 = x * x + y * y
        keep = finite & (cfg.lo2 <= r2) & (r2 < cfg.e2[cfg.n_ring])
        ring = np.zeros(len(p), np.int64)
        for k in range(1, cfg.n_ring):
            ring += r2 >= cfg.e2[k]
        upper = (y > 0) | ((y == 0) & (x > 0))
        xp, yp = np.where(upper, x, -x), np.where(upper, y, -y)
        sector = np.where(upper, 0, cfg.n_sector // 2).astype(np.int64)
        for k in range(1, cfg.n_sector // 2):
            sector += (cfg.bc[k] * yp - cfg.bs[k] * xp) >= 0
        v = z + np.float32(cfg.height_offset)
        keep &= v > 0
    return ring, sector, v, keep


def describe(cfg, pts):
    """(n_ring, n_sector) f32 descriptor of one scan."""
    ring, sector, v, keep = bins(cfg, pts)
    D = np.zeros((cfg.n_ring, cfg.n_sector), np.float32)
    np.maximum.at(D, (ring[keep], sector[keep]), v[keep])
    return D


def ring_key(D):
    return (np.asarray(D) > 0).sum(axis=-1).astype(np.int32)


def col_norms(D):
    D = np.asarray(D, np.float32)
    acc = np.zeros(D.shape[:-2] + D.shape[-1:], np.float64)
    for r in range(D.shape[-2]):
        d = D[..., r, :].astype(np.float64)
        acc = acc + d * d
    return np.sqrt(acc)


def distances(q, C):
    """q (NR, NS), C (N, NR, NS) -> d (N, NS) distance at every shift, ncol (N, NS)."""
    q = np.asarray(q, np.float32)
    C = np.asarray(C, np.float32).reshape((-1,) + q.shape)
    N, (NR, NS) = len(C), q.shape
    qn, Cn = col_norms(q), col_norms(C)
    q64, C64 = q.astype(np.float64), C.astype(np.float64)
    total = np.zeros((N, NS), np.float64)
    ncol = np.zeros((N, NS), np.int32)
    shifts = np.arange(NS)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(NS):
            cols = (j + shifts) % NS
            dot = np.zeros((N, NS), np.float64)
            for r in range(NR):
                dot = dot + q64[r, j] * C64[:, r, cols]
            valid = (qn[j] > 0) & (Cn[:, cols] > 0)
            term = 1.0 - dot / (qn[j] * Cn[:, cols])
            total = np.where(valid, total + term, total)
            ncol += valid
        d = np.where(ncol > 0, total / ncol, np.inf)
    return d, ncol


def ring_key_d2(q, C):
    a = ring_key(q).astype(np.int64)
    b = ring_key(np.asarray(C).reshape((-1,) + np.asarray(q).shape)).astype(np.int64)
    return ((a[None, :] - b) ** 2).sum(axis=1).astype(np.int32)


MATCH_FIELDS = ("index", "shift", "ring_key_d2", "n_columns", "distance")


def query(q, C, max_index=None, n_prefilter=0, k=1):
    """The k best of the entries C[:max_index] for the descriptor q: dict of arrays (k,), unused slots -1 / 0 / 0 / 0 / +inf.
    Also returns, under "all_distance", the best-shift distance of every compared candidate (for the separation asserts)."""
    q = np.asarray(q, np.float32)
    C = np.asarray(C, np.float32).reshape((-1,) + q.shape)
    n = len(C) if max_index is None else int(max_index)
    cand = np.arange(n)
    d2 = ring_key_d2(q, C[:n]) if n else np.zeros(0, np.int32)
    if n_prefilter > 0:
        cand = cand[np.argsort(d2, kind="stable")[:n_prefilter]]
    out = dict(index=np.full(k, -1, np.int32), shift=np.zeros(k, np.int32), ring_key_d2=np.zeros(k, np.int32),
               n_columns=np.zeros(k, np.int32), distance=np.full(k, np.inf))
    if len(cand) == 0:
        out["all_distance"] = np.zeros(0)
        return out
    cand = np.sort(cand)
    d, ncol = distances(q, C[cand])
    shift = np.argmin(d, axis=1)                       # first occurrence: the lowest shift that attains the minimum
    best = d[np.arange(len(cand)), shift]
    order = np.argsort(best, kind="stable")[:k]        # cand ascending + stable: (distance, index)
    m = len(order)
    out["index"][:m] = cand[order]
    out["shift"][:m] = shift[order]
    out["ring_key_d2"][:m] = d2[cand[order]]
    out["n_columns"][:m] = ncol[np.arange(len(cand)), shift][order]
    out["distance"][:m] = best[order]
    out["all_distance"] = best
    return out


def separated(dist, gap=1e-9):
    """The rule under which an index or shift comparison is meaningful: any two distances are bit-equal or more than `gap` apart."""
    d = np.sort(np.asarray(dist, np.float64)[np.isfinite(dist)])
    diff = np.diff(d)
    return bool(np.all((diff == 0) | (diff > gap)))


def place_yaw(shift, n_sector):
    a = 2.0 * np.pi * (np.asarray(shift) % n_sector) / n_sector
    return np.where(a > np.pi, a - 2.0 * np.pi, a)
