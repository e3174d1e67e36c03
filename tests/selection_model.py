"""The corner / flat selection of k_ring_features as Python: the reference's sequential walk (`literal`), the speculative
per-sector scheme the kernel runs (`model` over `pick_sector`) and its register-level form (`pick_sector_regs`).  Shared by
test_selection_model.py (the scheme against the definition on random rings) and selection_cases.py (rings built to force
named paths of the device code)."""
import numpy as np


def literal(curv, gap, n):
    """-> (labels, per-sector pick lists) by the reference's sequential walk.  gap[i]: the step i -> i+1 is longer than the
    0.05 threshold.  Ties: ascending (curvature, index), the canonical order (oracle default and the HIP path)."""
    L = n - 11
    picked = np.zeros(n, bool); label = np.zeros(n, np.int8); out = []
    for j in range(6):
        sp, ep = 5 + (L * j) // 6, 5 + (L * (j + 1)) // 6 - 1
        order = sorted(range(sp, ep + 1), key=lambda i: (curv[i], i))
        corners, flats = [], []
        def mark(ind):
            picked[ind] = True
            for l in range(1, 6):
                if gap[ind + l - 1]: break
                picked[ind + l] = True
            for l in range(-1, -6, -1):
                if gap[ind + l]: break
                picked[ind + l] = True
        cnt = 0
        for ind in reversed(order):
            if not picked[ind] and float(curv[ind]) > 0.1:
                cnt += 1
                if cnt <= 2: label[ind] = 2
                elif cnt <= 20: label[ind] = 1
                else: break
                corners.append(ind)
                mark(ind)
        cnt = 0
        for ind in order:
            if not picked[ind] and float(curv[ind]) < 0.1:
                label[ind] = -1
                flats.append(ind)
                cnt += 1
                if cnt >= 4: break
                mark(ind)
        out.append((corners, flats))
    return label, out


def pick_sector(j, init_marks, L, curv, reach):
    """One sector on its own: iterative arg-max / arg-min over the still-unpicked points.  -> corners, flats, spill mask."""
    sp, ln = (L * j) // 6, (L * (j + 1)) // 6 - (L * j) // 6
    first, last = sp + 5, sp + ln - 1 + 5
    alive = [not (p < 5 and (init_marks >> p) & 1) for p in range(ln)]
    spill = 0
    def pick_at(pos):
        nonlocal spill
        fw, bk = reach[first + pos]
        for q in range(max(0, pos - bk), min(ln - 1, pos + fw) + 1):
            alive[q] = False
        kf = first + pos
        for off in range(1, fw + 1):
            if kf + off > last:
                spill |= 1 << (kf + off - last - 1)
        return kf
    corners, flats = [], []
    count = 0
    while True:
        cand = [(curv[first + p], p) for p in range(ln) if alive[p] and curv[first + p] != 0]
        if not cand: break
        c, p = max(cand)                                                     # ties: the larger index
        if not float(c) > 0.1: break
        count += 1
        if count > 20: break
        corners.append(pick_at(p))
    count = 0
    while True:
        cand = [(curv[first + p], p) for p in range(ln) if alive[p]]
        if not cand: break
        c, p = min(cand)                                                     # ties: the smaller index
        if not float(c) < 0.1: break
        flats.append(first + p)
        count += 1
        if count >= 4: break
        pick_at(p)
    return corners, flats, spill


THR = int(np.float32(0.1).view(np.uint32))           # kCurvThresholdBits
INF = 0x7f800000


def pick_sector_regs(j, init_marks, L, curv, reach, W=64, spare=1):
    """pick_sector as the kernel evaluates it since round 3 (ALOAM_RF_PICK 2): point `pos` of the sector in register pos // W of lane
    pos % W; "dead" folded into the key (corner walk: curvature bits + 1, 0 = dead; flat walk: curvature bits, 0xffffffff = dead); the
    0.1 thresholds as integer compares on the bits; a pick kills through lane ranges of register kr and, when the range leaves
    0 .. W-1, of the register before or behind; the corner walk ends after the 20th pick.  W = 16 or 32 instead of 64 makes the
    register borders frequent."""
    sp, ln = (L * j) // 6, (L * (j + 1)) // 6 - (L * j) // 6
    first = sp + 5
    K = (ln + W - 1) // W + spare
    M32 = 0xffffffff
    cc = np.zeros((K, W), np.int64)
    for pos in range(ln):
        if not (pos < 5 and (init_marks >> pos) & 1):
            cc[pos // W, pos % W] = int(np.float32(curv[first + pos]).view(np.uint32)) + 1
    spill = 0
    lanes = np.arange(W)
    def kill(kr, f, dead):
        nonlocal spill
        fw, bk = reach[first + kr * W + f]
        P, lo, w = kr * W + f, f - bk, fw + bk
        cc[kr, ((lanes - lo) & M32) <= w] = dead
        if (lo & M32) > ((W - 1 - w) & M32):
            if lo < 0 and kr > 0: cc[kr - 1, lanes >= W + lo] = dead
            if lo >= 0 and kr + 1 < K: cc[kr + 1, lanes <= lo + w - W] = dead
        if P + 5 >= ln:
            e = P + fw - (ln - 1)
            if e > 0: spill |= (1 << e) - 1
        return P
    corners, flats = [], []
    for count in range(20):
        m = cc.max(axis=0)
        krl = np.zeros(W, np.int64)
        for r in range(1, K): krl = np.where(cc[r] == m, r, krl)
        cmax = int(m.max())
        if not (THR <= ((cmax - 1) & M32) <= INF): break
        tie = np.flatnonzero(m == cmax)
        f = int(tie[0]); kr = int(krl[f])
        if len(tie) != 1:
            wv = int(np.where(m == cmax, krl * W + lanes, 0).max()); f, kr = wv % W, wv // W
        corners.append(first + kill(kr, f, 0))
    cc = (cc - 1) & M32
    count = 0
    while True:
        m = cc.min(axis=0)
        krl = np.full(W, K - 1, np.int64)
        for r in range(K - 2, -1, -1): krl = np.where(cc[r] == m, r, krl)
        cmin = int(m.min())
        if not cmin < THR: break
        tie = np.flatnonzero(m == cmin)
        f = int(tie[0]); kr = int(krl[f])
        if len(tie) != 1:
            wv = int(np.where(m == cmin, krl * W + lanes, M32).min()); f, kr = wv % W, wv // W
        flats.append(first + kr * W + f)
        count += 1
        if count >= 4: break
        kill(kr, f, M32)
    return corners, flats, spill


def model(curv, gap, n, pick_sector=pick_sector):
    L = n - 11
    reach = []
    for i in range(n):
        fw = bk = 0
        while fw < 5 and i + fw < n - 1 and not gap[i + fw]: fw += 1
        while bk < 5 and i - 1 - bk >= 0 and not gap[i - 1 - bk]: bk += 1
        reach.append((fw, bk))
    res = [pick_sector(j, 0, L, curv, reach) for j in range(6)]              # concurrently, no incoming marks
    carry = res[0][2]
    for j in range(1, 6):
        sp, ln = (L * j) // 6, (L * (j + 1)) // 6 - (L * j) // 6
        m = carry if ln >= 5 else carry & ((1 << ln) - 1)
        if m:
            hit = any(pk - 5 - sp < 5 and (m >> (pk - 5 - sp)) & 1 for pk in res[j][0] + res[j][1])
            if hit:
                res[j] = pick_sector(j, m, L, curv, reach)
        carry = (0 if ln >= 5 else carry >> ln) | res[j][2]
    label = np.zeros(n, np.int8)
    for corners, flats, _ in res:
        for q, ind in enumerate(corners): label[ind] = 2 if q < 2 else 1
        for ind in flats: label[ind] = -1
    return label, [(c, f) for c, f, _ in res]
