"""CPU only (numpy). The pair kernels' trips know no range bound (pt_trace.h: trace_pair_flat, BOUND): a trip
accepts every positive finite t, and the ray's owner compares the minimum of the accepted t with the ray's bound once. This states
both acceptance rules on bit patterns, as the kernel does, and checks on random sets that they are the same predicate:

  old   exists t with f2u(t) - 1 < f2u(b') - 1 (unsigned, wrapping), b' = b if b > 0 else the smallest positive float
  new   m = min{f2u(t) : f2u(t) - 1 < 0x7f7fffff} exists and float(m) < b

and, for the extension ray (b = 999999, or any bound), that whenever the old rule has a hit both give the same minimum and the
same tied set (the t equal to the minimum)."""
import numpy as np

N_CASES = 120000          # >= 10^5
MAX_SET = 12
TINY = np.uint32(1)       # the smallest positive float's bit pattern
FINITE1 = np.uint32(0x7f7fffff)
SPECIAL = np.array([0x00000000, 0x80000000,                      # +0, -0
                    0x00000001, 0x007fffff, 0x80000001, 0x807fffff,      # denormals of both signs
                    0x00800000, 0x7f7fffff, 0xff7fffff,                  # smallest normal, largest finite, its negative
                    0x7f800000, 0xff800000,                              # +inf, -inf
                    0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fffffff, 0xff800001,      # NaNs of both signs
                    0x3f800000, 0xbf800000], np.uint32)
B999999 = np.float32(999999.0).view(np.uint32)


def _sets(rng):
    """(T [N, 12] uint32 bit patterns, valid [N, 12] bool, B [N] uint32 bound bit patterns)."""
    n = N_CASES
    kind = rng.integers(0, 6, n)
    pos = ((rng.integers(1, 0x7f800000, n, dtype=np.int64)).astype(np.uint32))            # a positive finite float, any exponent
    near = (np.float32(1.0) + rng.random(n, dtype=np.float32) * np.float32(1e6)).view(np.uint32)
    B = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [pos, near, np.full(n, B999999), np.full(n, 0x7f800000, np.uint32), SPECIAL[rng.integers(0, len(SPECIAL), n)]],
                  default=(rng.integers(0, 1 << 32, n, dtype=np.int64)).astype(np.uint32))    # any pattern: negatives, NaNs, ...
    B = B.astype(np.uint32)
    count = rng.integers(1, MAX_SET + 1, n)
    valid = np.arange(MAX_SET)[None, :] < count[:, None]
    how = rng.integers(0, 8, (n, MAX_SET))
    anyp = (rng.integers(0, 1 << 32, (n, MAX_SET), dtype=np.int64)).astype(np.uint32)
    step = rng.integers(-3, 4, (n, MAX_SET)).astype(np.int64)
    around = ((B[:, None].astype(np.int64) + step) & 0xffffffff).astype(np.uint32)      # both sides of the bound, a few ulps, and equal to it
    with np.errstate(all="ignore"):
        below = (B.view(np.float32)[:, None] * rng.random((n, MAX_SET), dtype=np.float32)).view(np.uint32)      # a fraction of the bound
    T = np.select([how == 0, how == 1, how == 2, how == 3, how == 4],
                  [anyp, around, below, SPECIAL[rng.integers(0, len(SPECIAL), (n, MAX_SET))], np.broadcast_to(B[:, None], (n, MAX_SET))],
                  default=(rng.integers(1, 0x7f800000, (n, MAX_SET), dtype=np.int64)).astype(np.uint32))
    return T.astype(np.uint32), valid, B


def _old_rule(T, valid, B):
    b = B.view(np.float32)
    with np.errstate(invalid="ignore"):
        Bp = np.where(b > 0, B, TINY).astype(np.uint32)              # (NaN > 0 is false)
    acc = ((T - np.uint32(1)) < (Bp - np.uint32(1))[:, None]) & valid      # uint32 arithmetic wraps
    return acc


def _new_rule(T, valid, B):
    acc = ((T - np.uint32(1)) < FINITE1) & valid
    m = np.where(acc, T, np.uint32(0xffffffff)).min(axis=1)          # the LDS minimum's high word: ~0u when nothing was accepted
    with np.errstate(invalid="ignore"):
        hit = m.view(np.float32) < B.view(np.float32)                # ~0u is a NaN: false
    return acc, m, hit


def test_the_unsigned_compare_accepts_exactly_the_positive_finite():
    T = np.concatenate([SPECIAL, np.random.default_rng(5).integers(0, 1 << 32, 200000, dtype=np.int64).astype(np.uint32)])
    t = T.view(np.float32)
    with np.errstate(invalid="ignore"):
        want = (t > 0) & np.isfinite(t)
    assert np.array_equal((T - np.uint32(1)) < FINITE1, want)


def test_both_rules_are_one_predicate_and_one_minimum():
    rng = np.random.default_rng(20260808)
    T, valid, B = _sets(rng)
    assert len(B) >= 100000
    old = _old_rule(T, valid, B)
    acc, m, hit = _new_rule(T, valid, B)
    old_hit = old.any(axis=1)
    # what the old rule says is what `0 < t < b` says, value by value (the proof next to `put`)
    t, b = T.view(np.float32), B.view(np.float32)
    with np.errstate(invalid="ignore"):
        plain = (t > 0) & (t < b[:, None]) & valid
    assert np.array_equal(old, plain)
    print("cases %d, hits under the old rule %d, sets with an accepted t beyond the bound %d" %
          (len(B), int(old_hit.sum()), int((acc & ~old).any(axis=1).sum())))
    assert old_hit.sum() > 10000 and (~old_hit).sum() > 10000 and (acc & ~old).any(axis=1).sum() > 10000
    assert np.array_equal(hit, old_hit)                               # the shadow ray's occlusion, and the extension ray's "hit or miss"
    # the extension form: the same minimum and the same tied set wherever the old rule has a hit
    m_old = np.where(old, T, np.uint32(0xffffffff)).min(axis=1)
    assert np.array_equal(m[old_hit], m_old[old_hit])
    tied_old = old & (T == m_old[:, None])
    tied_new = acc & (T == m[:, None])
    assert np.array_equal(tied_new[old_hit], tied_old[old_hit]) and tied_old[old_hit].any(axis=1).all()
    assert (tied_old[old_hit].sum(axis=1) > 1).sum() > 100          # (ties do occur in the sets)


def test_the_bounds_the_kernel_uses():
    """999999 (the extension ray), and every special bound, against every special t alone and in pairs."""
    S = SPECIAL
    Bs = np.concatenate([S, [B999999]]).astype(np.uint32)
    T1 = np.concatenate([S, [B999999, B999999 - 1, B999999 + 1]]).astype(np.uint32)
    a, c = np.meshgrid(T1, T1, indexing="ij")
    pairs = np.stack([a.ravel(), c.ravel()], axis=1)
    for bb in Bs:
        B = np.full(len(pairs), bb, np.uint32)
        valid = np.ones(pairs.shape, bool)
        old = _old_rule(pairs, valid, B)
        acc, m, hit = _new_rule(pairs, valid, B)
        assert np.array_equal(hit, old.any(axis=1)), hex(int(bb))
        oh = old.any(axis=1)
        m_old = np.where(old, pairs, np.uint32(0xffffffff)).min(axis=1)
        assert np.array_equal(m[oh], m_old[oh]), hex(int(bb))
        assert np.array_equal((acc & (pairs == m[:, None]))[oh], (old & (pairs == m_old[:, None]))[oh]), hex(int(bb))
