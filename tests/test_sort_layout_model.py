"""Model checks of the run-key sort of k_ring_features (aloam_device.hpp: bitonic_sort_blocked), run thread by thread in Python on
the key array as the kernel holds it:

  * network model: the all-ascending bitonic network with every half-cleaner register-blocked - strides (4 S, 2 S, S) on the eight
    keys i0 + u S of a thread, S = 1, 8, 64, 512, the topmost group of a merge holding one to three strides - sorts, with the
    slots n .. CAP - 1 holding garbage that the unguarded reads must replace by +inf and the unguarded writes may overwrite;
  * bank model: every LDS access of the sort is recorded as (pattern, key index per thread) and judged by the bank rule of the
    LDS - a wave64 access is served in fixed lane groups, and within a group every further distinct address on a busy bank costs
    one more cycle (RULE below: lane groups and banks per instruction kind, EMITTED: the instructions the compiler emits for each
    pass).  The array that ships is the plain one: the passes at S = 64 and 512 and the flips from k = 64 on are conflict-free,
    S = 1 travels as 16-byte accesses and is 2-way (4-way with 64-bit keys), S = 8 is 4-way (2-way).  The padded array (key i in dword i + (i >> 5), blocks of 64 dealt to the
    half-waves four apart) that makes all of them conflict-free for 32-bit keys was measured and lost to its index arithmetic
    (HISTORY.md); its claim is kept here as a model so that the record can be checked.
"""
import numpy as np
import pytest

NT = 256                     # threads of the workgroup


def pow2ceil(v):
    p = 1
    while p < v: p <<= 1
    return p


def _cx(v, a, b):
    lo, hi = np.minimum(v[:, a], v[:, b]), np.maximum(v[:, a], v[:, b])
    v[:, a], v[:, b] = lo, hi


def blocked_sort_model(keys, cap, inf, garbage_seed=1, trace=None):
    """bitonic_sort_blocked<K, cap>; trace collects (pattern, u, key index per thread or -1) per key access."""
    n = len(keys)
    npad = pow2ceil(n)
    arr = np.random.default_rng(garbage_seed).integers(0, inf, cap, dtype=np.uint64)   # whatever region A held before
    arr[:n] = np.asarray(keys, np.uint64)
    tid = np.arange(NT)

    def rec(pattern, u, idx, active):
        if trace is not None: trace.append((pattern, u, np.where(active, idx, -1)))

    def pass_of_eight(S, stages, first):
        U = 8 if 8 * S <= cap else cap // S
        q = tid.copy()
        while True:
            act = (q & ~(S - 1)) * 8 < n
            if not act.any(): break
            i0 = (q & ~(S - 1)) * 8 + (q & (S - 1))
            v = np.full((NT, 8), inf, np.uint64)
            for u in range(U):
                i = i0 + u * S
                assert (i[act] < cap).all()
                rec(f"S{S}", u, i, act)
                v[:, u] = np.where(i >= n, np.uint64(inf), arr[np.where(act, i, 0)])   # unguarded read, +inf behind n
            if first:
                for b in range(0, 8, 2): _cx(v, b, b + 1)
                for b in range(0, 8, 4): _cx(v, b, b + 3); _cx(v, b + 1, b + 2)
                for b in range(0, 8, 2): _cx(v, b, b + 1)
                for o in range(4): _cx(v, o, 7 - o)
            elif stages == 3:
                for o in range(4): _cx(v, o, o + 4)
            if stages >= 2:
                for b in range(0, 8, 4): _cx(v, b, b + 2); _cx(v, b + 1, b + 3)
            for b in range(0, 8, 2): _cx(v, b, b + 1)
            for u in range(U):
                i = i0 + u * S
                rec(f"S{S}", u, i, act)
                arr[i[act]] = v[act, u]                                      # unguarded write
            q += NT

    def level(S, stages):
        if stages >= 1: pass_of_eight(S, min(stages, 3), False)

    pass_of_eight(1, 3, True)
    lk = 4
    while (1 << lk) <= npad:
        k, hk = 1 << lk, 1 << (lk - 1)
        for t0 in range(0, npad >> 1, NT):                                    # flip
            t = t0 + tid
            off = t & (hk - 1)
            i = ((t - off) << 1) + off
            l = i + (k - 1 - 2 * off)
            act = (t < (npad >> 1)) & (l < n)
            rec("flip" if hk >= 32 else "narrow flip", 0, i, act); rec("flip" if hk >= 32 else "narrow flip", 0, l, act)
            x, y = arr[np.where(act, i, 0)], arr[np.where(act, l, 0)]
            sw = act & (x > y)
            arr[i[sw]], arr[l[sw]] = y[sw], x[sw]
        if cap >= 2048: level(512, lk - 10)
        level(64, lk - 7)
        level(8, lk - 4)
        pass_of_eight(1, 3, False)
        lk += 1
    return [int(x) for x in arr[:n]]


# ------------------------------------------------------------------------------------------------ network
SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 842, 1023, 1024, 1025, 2047, 2048]
INF32, INF64 = 0xffffffff, 0xffffffffffffffff


def _keys(kind, n, rng, inf):
    if kind == "random": return rng.integers(0, inf, n, dtype=np.uint64).tolist()
    if kind == "equal_high": return ((rng.integers(0, 3, n) << 12) | rng.permutation(n)).tolist()      # few voxels, distinct elements
    if kind == "ascending": return (np.arange(n) * 3 + 1).tolist()
    return (np.arange(n)[::-1] * 3 + 1).tolist()


@pytest.mark.parametrize("kind", ["random", "equal_high", "ascending", "descending"])
@pytest.mark.parametrize("cap,inf", [(2048, INF32), (2048, INF64), (4096, INF32)])
def test_blocked_network_sorts(kind, cap, inf):
    rng = np.random.default_rng(17)
    for n in SIZES + ([2049, 3000, 4095, 4096] if cap == 4096 else []):
        keys = _keys(kind, n, rng, inf)
        assert blocked_sort_model(keys, cap, inf, garbage_seed=n + 1) == sorted(keys), (kind, cap, n)


# ------------------------------------------------------------------------------------------------ bank rule
H32 = [range(0, 32), range(32, 64)]
Q16 = [range(g, g + 16) for g in range(0, 64, 16)]
B128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
RULE = {                     # kind -> (lane groups of a wave, banks, dwords per lane)
    "b32": (H32, 32, 1),                                                      # ds_read_b32, ds_read2_b32 (as two), ds_write_b32, ds_write2_b32
    "read_b64": (H32, 64, 2),
    "b64x": (Q16, 32, 2),                                                     # ds_write_b64, ds_read2_b64 / ds_write2_b64 (each of the two accesses)
    "read_b128": (B128 + [[l + 32 for l in g] for g in B128], 64, 4),
    "write_b128": ([range(g, g + 8) for g in range(0, 64, 8)], 32, 4),
}
# what hipcc -O3 emits for the sort (`-S`, between the after_run_heads and after_sort markers), per pass and key width: the S = 1
# pass moves a thread's 32 (64) contiguous bytes as two (four) 16-byte accesses, the strided passes use the two-address forms
EMITTED = {4: {"S1": ("read_b128", "write_b128", 4), "S8": ("b32", "b32", 1), "S64": ("b32", "b32", 1), "S512": ("b32", "b32", 1),
               "flip": ("b32", "b32", 1), "narrow flip": ("b32", "b32", 1)},
           8: {"S1": ("read_b128", "write_b128", 2), "S8": ("b64x", "b64x", 1), "S64": ("b64x", "b64x", 1), "S512": ("b64x", "b64x", 1),
               "flip": ("read_b64", "b64x", 1), "narrow flip": ("read_b64", "b64x", 1)}}


def multiplicity(kind, addr):
    """worst number of distinct addresses on one bank within a lane group, over the waves of the workgroup; addr < 0 = lane off"""
    groups, banks, width = RULE[kind]
    worst = 0
    for w in range(0, len(addr), 64):
        for grp in groups:
            per_bank = {}
            for lane in grp:
                a = int(addr[w + lane])
                if a < 0: continue
                for d in range(width): per_bank.setdefault((a + d) % banks, set()).add(a + d)
            worst = max([worst] + [len(s) for s in per_bank.values()])
    return worst


def worst_by_pattern(trace, key_bytes):
    """{pattern: (worst read multiplicity, worst write multiplicity)} under the instructions of EMITTED"""
    out = {}
    for pattern, u, idx in trace:
        rd, wr, keys_per_access = EMITTED[key_bytes][pattern]
        if u % keys_per_access: continue                                     # this key travels with the access of key u - u % keys_per_access
        addr = np.where(idx >= 0, idx * (key_bytes // 4), -1)
        r, w = out.get(pattern, (0, 0))
        out[pattern] = (max(r, multiplicity(rd, addr)), max(w, multiplicity(wr, addr)))
    return out


@pytest.mark.parametrize("n", [842, 1024, 2048])
def test_bank_conflicts_of_the_plain_array(n):
    trace = []
    keys = np.random.default_rng(n).permutation(n).tolist()
    assert blocked_sort_model(keys, 2048, INF32, trace=trace) == sorted(keys)
    w4, w8 = worst_by_pattern(trace, 4), worst_by_pattern(trace, 8)
    want4 = {"S1": (2, 2), "S8": (4, 4), "S64": (1, 1), "flip": (1, 1), "narrow flip": (2, 2)}
    want8 = {"S1": (4, 4), "S8": (2, 2), "S64": (1, 1), "flip": (1, 1), "narrow flip": (2, 2)}
    if n == 2048: want4["S512"] = want8["S512"] = (1, 1)
    assert w4 == want4 and w8 == want8


def test_padded_array_would_be_conflict_free_for_32_bit_keys():
    """the rejected layout: key i in dword i + (i >> 5); at S = 8 the four blocks of a half-wave are taken four apart
    (66 dwords per block of 64 keys, 4 x 66 = 8 mod 32).  (a) S = 1, (b) S = 8, (c) 64 consecutive keys per wave."""
    slot = lambda i: i + (i >> 5)
    tid = np.arange(NT)
    g = tid >> 3
    block = ((g & 3) << 2) | ((g >> 2) & 3) | (g & 16)
    assert sorted(set(block.tolist())) == list(range(32))
    for u in range(8):
        assert multiplicity("b32", slot(tid * 8 + u)) == 1 and multiplicity("b32", tid * 8 + u) == 8   # (a): the pads leave only 4-byte accesses
        assert multiplicity("b32", slot(block * 64 + (tid & 7) + 8 * u)) == 1                    # (b), swizzled blocks
        assert multiplicity("b32", slot((tid >> 3) * 64 + (tid & 7) + 8 * u)) == 4               # (b), consecutive blocks: pads alone do not help
    assert multiplicity("b32", slot(tid)) == 1 and multiplicity("b32", slot(2047 - tid)) == 1    # (c)
    # room: the 32-bit keys fit the 8 * NPAD bytes region A gives the run keys, 64-bit keys with one pad per 32 do not fit 8 * NPAD + 128
    for npad in (2048, 4096):
        assert 4 * slot(npad) <= 8 * npad and 8 * slot(npad) > 8 * npad + 128
