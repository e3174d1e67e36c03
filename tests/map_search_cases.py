"""A constructed map and stack for the scan-to-map search and fit (a-loam_amd/csrc/mapping_kernels.hip k_mapgrid_build / k_map_search / k_map_fit,
map_search_device.hpp), with the facts that show which path each query is there for.  No GPU in here.

Everything is built in the map frame and run at the identity pose, so a stack point IS its pointSel and dyadic coordinates stay exact.  The map
reaches the oracle the only way it takes one, through mapping steps: frame A at the origin carries the bulk (each point alone in its 1/16 m voxel, so
the stack filter and the cube filter hand it on as it is), frames B1 .. B4, 200 m away, carry the duplicates - their points land in the cube around the
origin, which is outside those frames' window and therefore not filtered again, so identical points survive under different indices.  The library gets
the oracle's cubes through set_map / set_map_frame; both then take the test frame.  The model of a factor record is factors_by_query(): the five
nearest of the oracle's own from-map cloud in its order, then the oracle's Eigen stand-ins, in the style of loopreg_model.factors (asserted equal to
it); define5() is the plain definition of the five with the plausible mistakes as switches, fit_numpy() the independent f64 evaluation that measures
how far the stand-ins sit from another algorithm.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle_py
from assoc_cases import dist2

F = np.float32
LEAF = 0.0625                                          # both classes: every constructed point is alone in its voxel
POOL_POINTS = 65536
FAR = np.array([200.0, 0.0, 0.0])                      # where the duplicate frames are taken from: four cubes off the window's centre
SITES = (-20.0, -12.0, -4.0, 4.0, 12.0, 20.0)          # case sites: even coordinates (2 m cell borders), 8 m apart, never 0, all in the cube around the origin


def table_size(pool_points):
    """map_alloc_pool (capi_mapping.hip): the bucket table follows the pool, 4096 .. kMapGridMaxH = 32768."""
    H = 4096
    while H < pool_points // 16 and H < 32768:
        H <<= 1
    return H


def cell_of(p):
    """floor(x * 0.5f) per axis: the 2 m cell of k_mapgrid_build / k_map_search."""
    return np.floor(np.asarray(p, F)[..., :3] * F(0.5)).astype(np.int64)


def map_bucket(x, y, z, H):
    """map_bucket() of map_search_device.hpp: parities of the cell in the low three bits, hash of the 4 m super-cell above them."""
    m = 0xFFFFFFFF
    x, y, z = int(x), int(y), int(z)
    h = ((((x >> 1) & m) * 73856093 & m) ^ (((y >> 1) & m) * 19349663 & m) ^ (((z >> 1) & m) * 83492791 & m))
    return ((h << 3 & m) | (x & 1) | ((y & 1) << 1) | ((z & 1) << 2)) & (H - 1)


def block_of(sel, wrong_side=False):
    """The eight cells k_map_search walks: the own cell and per axis the neighbour on the side of the cell the query sits in (>= 0.5: above)."""
    g = np.asarray(sel, F)[:3] * F(0.5)
    c = np.floor(g).astype(np.int64)
    up = (g - c.astype(F)) >= F(0.5)
    if wrong_side:
        up = ~up
    nb = np.where(up, c + 1, c - 1)
    return [tuple(int(nb[a]) if m >> a & 1 else int(c[a]) for a in range(3)) for m in range(8)]


# ---- the definition and the model ------------------------------------------------------------------------------------------------------------------
def define5(tgt, sel, highest=False, le=False, sixth=False, wrong_side=False):
    """The five neighbours the reference uses (nearestKSearch(k = 5), kept if the fifth is closer than 1 m; src/laserMapping.cpp:582,650), ties to the
    lowest index; None = not found.  Mistakes: `highest` - ties to the highest index; `le` - d <= 1; `sixth` - the sixth neighbour in the fifth's
    place; `wrong_side` - only the 2x2x2 block with the neighbour cells on the wrong side is looked at."""
    d = dist2(tgt, sel)
    idx = np.arange(len(tgt))
    if wrong_side:
        cells = cell_of(tgt)
        keep = np.zeros(len(tgt), bool)
        for c in block_of(sel, True):
            keep |= np.all(cells == c, axis=1)
        idx = idx[keep]
    order = idx[np.lexsort((-idx if highest else idx, d[idx]))]
    need = 6 if sixth else 5
    if len(order) < need:
        return None
    five = list(order[:4]) + [order[5 if sixth else 4]]
    last = d[five[4]]
    return [int(i) for i in five] if (last <= F(1.0) if le else last < F(1.0)) else None


def fit_oracle(cls, near):
    """The record of five neighbours [5, 3] f64 by the oracle's Eigen stand-ins: corner (a, b) or None; surf (n, d), kept unless a residual exceeds 0.2
    (a NaN does not: reference :672-678 asks `> 0.2`)."""
    if cls == 0:
        c = np.zeros(3)
        for j in range(5):
            c = c + near[j]
        c = c / 5.0
        cov = np.zeros((3, 3))
        for j in range(5):
            z = near[j] - c
            cov = cov + np.outer(z, z)
        vals, vecs = oracle_py.sym_eigen3(cov)
        if not vals[2] > 3 * vals[1]:
            return None
        d = vecs[:, 2]
        return np.concatenate([0.1 * d + c, -0.1 * d + c])
    x = oracle_py.lstsq_5x3(near, -np.ones(5))
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        d, n = np.float64(1.0) / ln, x / ln
        if any(abs(n[0] * p[0] + n[1] * p[1] + n[2] * p[2] + d) > 0.2 for p in near):
            return None
    return np.concatenate([n, [d]])


def _basic_lstsq(A, b):
    """min |A x - b| as colPivHouseholderQr().solve() defines it for any rank - pivot columns by largest remaining norm, the others 0 - with the
    numbers from numpy.linalg.lstsq on the chosen columns."""
    rest, cols = A.copy(), []
    first = None
    for _ in range(3):
        norms = (rest * rest).sum(axis=0)
        norms[cols] = -1.0
        j = int(np.argmax(norms))
        first = norms[j] if first is None else first
        if not norms[j] > first * 1e-20:
            break
        cols.append(j)
        q = rest[:, j] / math.sqrt(norms[j])
        rest = rest - np.outer(q, q @ rest)
    x = np.zeros(3)
    if cols:
        x[cols] = np.linalg.lstsq(A[:, cols], b, rcond=None)[0]
    return x


def fit_numpy(cls, near):
    """The same record by an independent f64 evaluation (numpy.linalg.eigh / lstsq); the decision is taken from it too."""
    if cls == 0:
        c = near.mean(axis=0)
        z = near - c
        vals, vecs = np.linalg.eigh(z.T @ z)
        if not vals[2] > 3 * vals[1]:
            return None
        return np.concatenate([0.1 * vecs[:, 2] + c, -0.1 * vecs[:, 2] + c])
    x = _basic_lstsq(near, -np.ones(5))
    ln = np.linalg.norm(x)
    n, d = x / ln, 1.0 / ln
    return None if (np.abs(near @ n + d) > 0.2).any() else np.concatenate([n, [d]])


def record_difference(cls, a, b):
    """Largest component difference of two records; a line as the unordered pair {a, b} (an eigenvector's sign is free)."""
    if cls == 0:
        return min(np.abs(a - b).max(), np.abs(a - np.concatenate([b[3:], b[:3]])).max())
    return np.abs(a - b).max()


def factors_by_query(cls, stack, tgt, knn=None, fit=fit_oracle, **mistake):
    """{stack index: (five indices, record)} of the queries that get a factor.  knn: (idx [n, 5], d2 [n, 5]) of oracle_py.knn_search, else define5."""
    out = {}
    for i, p in enumerate(stack):
        if knn is not None:
            five = [int(j) for j in knn[0][i]] if knn[0][i, 4] >= 0 and knn[1][i, 4] < F(1.0) else None
        else:
            five = define5(tgt, p[:3], **mistake)
        if five is not None:
            rec = fit(cls, tgt[five, :3].astype(np.float64))
            if rec is not None:
                out[i] = (five, rec)
    return out


# ---- building --------------------------------------------------------------------------------------------------------------------------------------
def five_set(cls, centre, axis=0, scale=1.0):
    """Five points within 0.32 scale of `centre`: corner class - along `axis` with a centimetre of jitter (a line whatever four or five of them are
    taken with); surf class - a pentagon in the plane normal to `axis`, a centimetre off it."""
    P = np.zeros((5, 3))
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    if cls == 0:
        P[:, a] = np.array([-0.3, -0.15, 0.0, 0.15, 0.3]) * scale
        P[:, b] = [0.010, -0.012, 0.004, 0.011, -0.008]
        P[:, c] = [-0.006, 0.009, 0.012, -0.010, 0.003]
    else:
        ang = np.deg2rad(72.0 * np.arange(5) + 11.0)
        P[:, b], P[:, c] = 0.2 * scale * np.cos(ang), 0.2 * scale * np.sin(ang)
        P[:, a] = [0.010, -0.012, 0.004, 0.011, -0.008]
    return P + np.asarray(centre, float)


class _Builder:
    def __init__(self):
        self.map = ([], [])                             # frame A
        self.dup = [([], []) for _ in range(4)]        # frames B1 .. B4
        self.q = ([], [])                               # (xyz, tag, expect found)
        self.site_no = 0

    def site(self):
        k = self.site_no
        self.site_no += 1
        assert k < 216
        k = k * 37 % 216                               # spread over the whole cube: both signs on every axis for either class
        return np.array([SITES[k % 6], SITES[(k // 6) % 6], SITES[k // 36]])

    def pts(self, cls, P, frame=None):
        for p in np.asarray(P, float).reshape(-1, 3):
            (self.map if frame is None else self.dup[frame])[cls].append(p)

    def query(self, cls, p, tag, expect):
        self.q[cls].append((np.asarray(p, float), tag, expect))


def _m1(b, cls):
    """The gate."""
    for rep in range(2):
        o = b.site()
        q = o + [0.7, 0.6, 0.5]
        P = five_set(cls, q + [0.1, 0.05, 0.02], axis=rep)
        b.pts(cls, P); b.pts(cls, q + [[0.0, 0.0, 1.3]])
        b.query(cls, q, "five-in-range", True)
        o = b.site()
        q = o + [0.7, 0.6, 0.5]
        b.pts(cls, five_set(cls, q + [0.1, 0.05, 0.02], axis=rep)[:4]); b.pts(cls, q + [[0.0, 1.2, 0.0]])
        b.query(cls, q, "four-in-range", False)
    # dyadic: four within 1 m and the fifth at exactly d2 = 1.0f; the query one ulp nearer
    four = [[0.25, 0, 0], [-0.25, 0, 0], [0.5, 0, 0], [-0.5, 0, 0]] if cls == 0 else [[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]
    for sign in (1.0, -1.0):
        for ulp, tag, expect in ((0.0, "fifth-at-exactly-1", False), (1.0, "fifth-one-ulp-inside", True)):
            o = b.site()
            q = o + [1.0, 0.5, 0.5]
            b.pts(cls, q + np.array(four + [[sign, 0, 0]]))
            qq = q.copy()
            qq[0] = float(np.nextafter(F(q[0]), F(q[0] + sign))) if ulp else q[0]
            b.query(cls, qq, tag, expect)


def _m2(b, cls):
    """Block choice: fractional positions 0, 0.5, just either side of 0.5 on each axis; the eight octants with the five in the diagonal neighbour cell."""
    for axis in range(3):
        for step, tag in ((None, "frac-0"), (0.0, "frac-0.5"), (-np.inf, "frac-just-below-0.5"), (np.inf, "frac-just-above-0.5")):
            o = b.site()
            q = o + [0.4, 0.4, 0.4]
            # the cell's lower border; its centre; the f32 neighbours of the centre
            q[axis] = o[axis] if step is None else o[axis] + 1.0 if step == 0.0 else float(np.nextafter(F(o[axis] + 1.0), F(step)))
            c = q.copy()
            c[axis] -= 0.35 if step is None else 0.0     # at fraction 0 the five lie in the cell below the query's
            b.pts(cls, five_set(cls, c, axis=axis))
            b.query(cls, q, tag, True)
    for m in range(8):
        s = np.array([1.0 if m >> a & 1 else -1.0 for a in range(3)])
        o = b.site()
        q = o + 1.0 + 0.8 * s                            # 0.2 m from three faces of its cell
        if cls == 0:
            P = q + np.outer([0.26, 0.33, 0.40, 0.47, 0.54], s) + np.array([[0.01, -0.01, 0.0], [-0.012, 0.0, 0.01], [0.0, 0.008, -0.01], [0.011, -0.006, 0.0], [0.0, 0.01, -0.012]])
        else:
            e1 = np.cross(s, [0.0, 0.0, 1.0]); e1 /= np.linalg.norm(e1)
            e2 = np.cross(s, e1); e2 /= np.linalg.norm(e2)
            ang = np.deg2rad(72.0 * np.arange(5) + 11.0)
            P = q + 0.36 * s + 0.12 * (np.outer(np.cos(ang), e1) + np.outer(np.sin(ang), e2)) + np.outer([0.004, -0.005, 0.002, 0.005, -0.003], s)
        b.pts(cls, P)
        b.query(cls, q, "octant-diagonal-cell", True)


def _m3(b, cls):
    """Ties."""
    for rep in range(3):                                 # four nearest, then eight equidistant points for the fifth place
        o = b.site()
        q = o + [1.0, 1.0, 0.5] + 0.25 * rep
        if cls == 0:
            near = [[sx * 0.125, sy * 0.0625, 0.0] for sx in (1, -1) for sy in (1, -1)]
            tied = [[sx * 0.375, sy * 0.0625, 0.0] for sx in (1, -1) for sy in (1, -1)] + [[sx * 0.375, 0.0, sz * 0.0625] for sx in (1, -1) for sz in (1, -1)]
        else:
            zs = (0.0625, -0.0625)
            near = [[sx * 0.125, sy * 0.125, zs[(sx + sy) // 2 % 2] * 0.5] for sx in (1, -1) for sy in (1, -1)]
            tied = [[sx * 0.375, sy * 0.125, zs[k % 2]] for k, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1)))] + \
                   [[sx * 0.125, sy * 0.375, zs[(k + 1) % 2]] for k, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1)))]
        order = np.random.default_rng(rep).permutation(len(tied))
        b.pts(cls, q + np.array(near)); b.pts(cls, q + np.array(tied)[order])
        b.query(cls, q, "eight-tied-for-fifth", True)
    for rep in range(2):                                 # identical points under different indices: three near points and one point twice -> five
        o = b.site()
        q = o + [0.6, 0.7, 0.5]
        P = np.round(five_set(cls, q + [0.1, 0.0, 0.05], axis=rep) * 1024.0) / 1024.0     # dyadic: the copy survives its trip through the far frame
        b.pts(cls, P[:4]); b.pts(cls, P[3:4], frame=0)
        b.query(cls, q, "a-point-twice-makes-five", True)
    for rep in range(2):                                 # a tie between entries of two buckets: the query on a cell border, the fifth place mirrored across it
        o = b.site()
        q = o + [0.0, 0.5 + 0.25 * rep, 0.5]
        if cls == 0:
            four = [[0.125, 0.0625, 0], [-0.125, 0.0625, 0], [0.25, -0.0625, 0], [-0.25, -0.0625, 0]]
            pair = [[0.5, 0, 0.0625], [-0.5, 0, 0.0625]]
        else:
            four = [[0.125, 0.25, 0.0], [-0.125, 0.25, 0.03125], [0.125, -0.25, 0.03125], [-0.125, -0.25, 0.0]]
            pair = [[0.5, 0, 0.0625], [-0.5, 0, 0.0625]]
        b.pts(cls, q + np.array(four)); b.pts(cls, q + np.array(pair if rep else pair[::-1]))
        b.query(cls, q, "tie-across-two-buckets", True)


def _split(P, axis, sign, border, k):
    """Move the set P along `axis` so that exactly k of its points lie on the near side of `border` (near: below it for sign > 0, above for sign < 0)."""
    v = np.sort(P[:, axis]) if sign > 0 else np.sort(P[:, axis])[::-1]
    cut = v[-1] + sign * 0.2 if k == len(P) else 0.5 * (v[k - 1] + v[k])
    P = P.copy()
    P[:, axis] += border - cut
    near = (P[:, axis] < border) if sign > 0 else (P[:, axis] >= border)
    assert near.sum() == k
    return P


def _m4(b, cls):
    """One 2 m cell of about 2000 points - rods along x (corner) / sheets z = const (surf), so that any five nearest are a line / a plane - and, next
    to it, cells of 1 .. 5 entries: each holds the near part of a five-set split over the cell's outer border, so the record needs every entry of the
    bucket (tails m = 1, 2, 3 of the four-loads-at-a-time walk; 1944 = 4 x 486, 1875 = 4 x 468 + 3).  Two more hold 3 and 2 entries of FOUR-point sets
    (3 | 1 and 2 | 2): four in range, no record - unless a tail entry were visited twice."""
    o = b.site()
    if cls == 0:
        big = np.array([[0.04 + 0.08 * i, 0.2 + 0.2 * j, 0.2 + 0.2 * k] for j in range(9) for k in range(9) for i in range(24)])      # 1944
    else:
        big = np.array([[0.04 + 0.08 * i, 0.04 + 0.08 * j, 0.4 + 0.6 * k] for k in range(3) for j in range(25) for i in range(25)])   # 1875
    b.pts(cls, o + big)
    for k, at in enumerate(([0.5, 0.6, 0.6], [1.31, 1.0, 1.4], [1.0, 1.8, 0.2], [0.45, 0.2, 1.8], [1.5, 1.4, 1.0], [0.77, 0.41, 0.98])):
        q = o + (np.array(at) if cls == 0 else np.array([at[0], at[1], 0.4 + 0.6 * (k % 3) + 0.03]))
        b.query(cls, q, "inside-the-long-bucket", True)

    def split_set(axis, sign, k, n, other, tag, expect):
        border = o[axis] + (4.0 if sign > 0 else -2.0)   # the outer border of the cell beside the big one
        centre = o + other
        centre[axis] = border
        P = five_set(cls, centre, axis=axis if cls == 0 else (axis + 1) % 3)[:n]    # spread along `axis`: the line itself / inside the pentagon's plane
        P = _split(P, axis, sign, border, k)
        b.pts(cls, P)
        b.query(cls, P.mean(axis=0) + 0.04, tag, expect)
    for k, (axis, sign) in zip(range(1, 6), ((0, -1), (1, 1), (1, -1), (2, 1), (2, -1))):
        split_set(axis, sign, k, 5, 1.0, f"needs-every-entry-of-a-{k}-bucket", True)
    split_set(0, 1, 3, 4, 1.0, "four-in-range-3-and-1", False)


def _m5(b, cls, H):
    """Cells far apart that share a bucket with a cell of a query's block: their entries are walked and must all fail d < 1.  Built last: a far cell is
    taken only two cells clear of everything else."""
    def occupied():
        occ = {tuple(c) for c in cell_of(np.array(b.map[cls] + [p for d in b.dup for p in d[cls]]))}
        for q, _, _ in b.q[cls]:
            occ |= set(block_of(q))
        return occ
    b.shared = getattr(b, "shared", {})
    for rep in range(3):
        o = b.site()
        q = o + [0.6, 0.7, 0.5]
        b.pts(cls, five_set(cls, q + [0.1, 0.0, 0.05], axis=rep))
        b.query(cls, q, "block-shares-buckets-with-far-cells", True)
        want = {map_bucket(*c, H): c for c in block_of(q)}
        occ = occupied()
        rng = np.random.default_rng(100 + rep)
        found = []
        for cx in range(-11, 11):
            for cy in range(-11, 11):
                for cz in range(-11, 11):
                    if len(found) < 4 and map_bucket(cx, cy, cz, H) in want and (cx + cy + cz) % 3 == rep and \
                       not any((cx + i, cy + j, cz + k) in occ for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)):
                        base = np.array([cx, cy, cz]) * 2.0
                        b.pts(cls, base + 0.1 + 0.15 * np.array([[i % 12, (i // 12) % 12, i // 144] for i in range(29)]) + 0.01 * rng.random((29, 3)))
                        found.append((cx, cy, cz))
                        occ.add((cx, cy, cz))
        assert len(found) >= 2, (cls, rep, found)
        b.shared[cls, tuple(np.round(q, 6))] = found


def _m6(b, cls):
    """Fits."""
    if cls == 0:
        o = b.site()
        q = o + [1.0, 0.5, 0.5]
        b.pts(cls, q + np.array([[0.25 * k, 0.125, 0.0] for k in (-2, -1, 0, 1, 2)]))
        b.query(cls, q, "five-collinear", True)
        o = b.site()
        q = o + [0.5, 0.5, 0.5]
        p = q + [0.25, 0.125, 0.0]
        b.pts(cls, [p])
        for f in range(4):
            b.pts(cls, [p], frame=f)
        b.query(cls, q, "five-identical", False)        # covariance 0: 0 > 3 * 0 is false
        o = b.site()
        q = o + [0.5, 0.5, 0.5]
        b.pts(cls, q + np.array([[0.3, 0, 0], [-0.3, 0, 0], [0, 0.3, 0], [0, -0.3, 0], [0, 0, 0.3]]))
        b.query(cls, q, "no-line", False)
    else:
        o = b.site()
        q = o + [1.0, 1.0, 0.5]
        b.pts(cls, q + np.array([[0.25, 0, 0.125], [-0.25, 0.125, 0.125], [0, 0.25, 0.125], [0.125, -0.25, 0.125], [-0.125, -0.125, 0.125]]))
        b.query(cls, q, "five-in-an-exact-plane", True)
        o = b.site()
        q = o + [0.5, 0.5, 0.5]
        p = q + [0.25, 0.125, 0.0]
        b.pts(cls, [p])
        for f in range(4):
            b.pts(cls, [p], frame=f)
        b.query(cls, q, "five-identical", True)         # rank 1: the plane through the point, normal along the pivot axis; residuals 0
        o = b.site()
        q = o + [0.5, 0.5, 0.5]
        b.pts(cls, q + np.array([[0.3, 0, 0.4], [-0.3, 0, 0.4], [0, 0.3, -0.4], [0, -0.3, -0.4], [0.1, 0.1, 0.0]]))
        b.query(cls, q, "plane-fails-0.2", False)


def _filler(b, cls):
    """Plain found / not-found queries that bring the frame to 20 records and 5 non-records per class and the map past the gate (> 10 corner, > 50 surf)."""
    for rep in range(6):
        o = b.site()
        q = o + [0.9, 1.1, 0.7]
        b.pts(cls, five_set(cls, q + [0.05, 0.1, -0.1], axis=rep % 3))
        b.pts(cls, q + [[0.5, 0.6, 0.45]])               # the sixth: in range, far off the line / plane
        b.query(cls, q, "sixth-in-range", True)
    for rep in range(3):
        o = b.site()
        b.query(cls, o + [1.0, 1.0, 1.0], "nothing-in-range", False)


@functools.lru_cache(maxsize=None)
def scene(origin_case=False):
    """The frame with M1 .. M6.  origin_case: instead, a small frame whose one surf query has five neighbours AT the origin (CPU only)."""
    b = _Builder()
    H = table_size(POOL_POINTS)
    if origin_case:
        for cls in (0, 1):
            _filler(b, cls)
            _m4(b, cls)                                  # (brings the surf class past the gate)
        b.pts(1, [[0.0, 0.0, 0.0]])
        for f in range(4):
            b.pts(1, [[0.0, 0.0, 0.0]], frame=f)
        b.query(1, [0.25, 0.125, 0.0], "five-at-the-origin", None)
    else:
        for cls in (0, 1):
            _m1(b, cls); _m2(b, cls); _m3(b, cls); _m4(b, cls); _m6(b, cls); _filler(b, cls); _m5(b, cls, H)
    s = SimpleNamespace(H=H, shared=getattr(b, "shared", {}))

    def cloud(pts):
        a = np.zeros((len(pts), 4), F)
        if len(pts):
            a[:, :3] = np.array(pts)
        return a
    s.map_frames = [(cloud(b.map[0]), cloud(b.map[1]), np.zeros(3))] + [(cloud(np.array(d[0]) - FAR if d[0] else []), cloud(np.array(d[1]) - FAR if d[1] else []), FAR) for d in b.dup]
    # the stack in the order the down-sizing filter emits it (voxel order); it must then pass the filter unchanged
    s.stack, s.tags, s.expect = [], [], []
    for cls in (0, 1):
        raw = cloud([q[0] for q in b.q[cls]])
        raw[:, 3] = np.arange(len(raw))                  # carries the construction index through the filter
        st = oracle_py.voxel_filter(raw, LEAF, canonical=True)
        order = st[:, 3].astype(int)
        s.stack.append(st)
        s.tags.append([b.q[cls][i][1] for i in order])
        s.expect.append([b.q[cls][i][2] for i in order])
    return s


def build_oracle(s, lm=0):
    """An oracle that holds the constructed map: (oracle, from-map clouds in submap order per class, its cubes per class)."""
    orc = oracle_py.Oracle(n_scans=16, min_range=0.3, lm_max_iterations=lm)
    orc.map_config(LEAF, LEAF)
    for corner, surf, t in s.map_frames:
        orc.mapping_step([0, 0, 0, 1.0], t, corner, surf, surf[:4])
    tgt, both = [], []
    for cls in (0, 1):
        cubes = orc.map_cubes(cls)
        order = sorted(cubes, key=lambda i: (i % 21, (i // 21) % 21, i // 441))
        tgt.append(np.concatenate([cubes[i] for i in order]) if order else np.zeros((0, 4), F))
        both.append(cubes)
    return orc, tgt, both


def step_oracle(orc, s):
    orc.mapping_step([0, 0, 0, 1.0], [0, 0, 0.0], s.stack[0], s.stack[1], s.stack[1][:4])
    return orc.map_info()


# ---- the model of the test frame, the tolerance, the comparison ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluated(origin_case=False):
    """Everything the tests need of the frame from the CPU alone, computed once: the oracle's map_info of the test frame, its decision log, the from-map
    clouds, and per class the model's records {stack index: (five, record)}."""
    s = scene(origin_case)
    orc, tgt, cubes = build_oracle(s)                   # the cubes as the test frame meets them (its own end re-filters them)
    oracle_py.decision_log(True)
    info = step_oracle(orc, s)
    kinds, values, thresholds = oracle_py.decisions()
    oracle_py.decision_log(False)
    model = []
    for cls in (0, 1):
        knn = oracle_py.knn_search(tgt[cls], s.stack[cls], 5)
        model.append(factors_by_query(cls, s.stack[cls], tgt[cls], knn=knn))
    return SimpleNamespace(scene=s, tgt=tgt, info=info, decisions=(kinds.copy(), values.copy(), thresholds.copy()), model=model,
                           cubes=cubes)


@functools.lru_cache(maxsize=None)
def measured_spread():
    """The largest difference, over the neighbour sets of these very cases, between a record by the oracle's Eigen stand-ins and by numpy's eigh / lstsq;
    both must take the same decision on every set."""
    ev = evaluated()
    worst = 0.0
    for cls in (0, 1):
        for i in range(len(ev.scene.stack[cls])):
            five = define5(ev.tgt[cls], ev.scene.stack[cls][i, :3])
            if five is None:
                continue
            near = ev.tgt[cls][five, :3].astype(np.float64)
            a, b = fit_oracle(cls, near), fit_numpy(cls, near)
            assert (a is None) == (b is None), (cls, i, ev.scene.tags[cls][i])
            if a is not None:
                worst = max(worst, float(record_difference(cls, a, b)))
    return worst


def device_tolerance():
    """What the device's line ends and plane (n, d) may deviate from the model: 100 times the measured spread - its Jacobi / Householder sequences are
    a third algorithm."""
    return 100.0 * measured_spread()


def compare_factors(ev, lines, planes, tol):
    """The device's map_factors against the model, record by record in stack order: cp bit for bit, a line as the unordered pair {a, b} and a plane's
    (n, d) within tol.  Returns {(class, tag): (queries, disagreeing)} and the largest deviation seen; raises nothing - the caller asserts."""
    out, worst, problems = {}, 0.0, []
    for cls, got in enumerate((lines, planes)):
        s, model = ev.scene, ev.model[cls]
        cp = {s.stack[cls][i, :3].astype(np.float64).tobytes(): i for i in range(len(s.stack[cls]))}
        seen = {}
        for r in got:
            i = cp.get(np.ascontiguousarray(r[:3]).tobytes())
            if i is None or i in seen:
                problems.append((cls, "cp is no stack point, or twice", r[:3].tolist()))
                continue
            seen[i] = r[3:]
        if sorted(seen) != [cp[np.ascontiguousarray(r[:3]).tobytes()] for r in got if np.ascontiguousarray(r[:3]).tobytes() in cp]:
            problems.append((cls, "records are not in stack order"))
        bad = set(seen) ^ set(model)
        for i in set(seen) & set(model):
            dev = float(record_difference(cls, model[i][1], seen[i]))
            worst = max(worst, dev)
            if not dev <= tol:
                bad.add(i)
                problems.append((cls, i, s.tags[cls][i], dev))
        for i in set(seen) ^ set(model):
            problems.append((cls, i, s.tags[cls][i], "record only on the device" if i in seen else "record only in the model"))
        for tag in sorted(set(s.tags[cls])):
            idx = [i for i, t in enumerate(s.tags[cls]) if t == tag]
            out[("corner", "surf")[cls], tag] = (len(idx), sum(1 for i in idx if i in bad))
    return out, worst, problems


INFO_KEYS = ("cenW", "cenH", "cenD", "frame_count", "from_map_corner", "from_map_surf", "corner_stack", "surf_stack", "corner_num0", "corner_num1", "surf_num0", "surf_num1")
MISTAKES = {"highest": dict(highest=True), "le": dict(le=True), "sixth": dict(sixth=True), "wrong_side": dict(wrong_side=True)}
SENSITIVITY = {"highest": 5, "le": 2, "sixth": 20, "wrong_side": 11}       # least number of queries per class whose record each mistake must change
