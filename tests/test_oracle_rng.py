"""XORWOW restatement: recurrence + 2^67 jump cross-checked against rocRAND's shipped table (its
matrices committed as tests/golden/rocrand_xorwow_tables.json, tests/golden/make_golden.py --rocrand),
and the committed KATs. The cuRAND scramble constants cannot be verified offline (PARITY UNPINNED)."""
import json
import os

import numpy as np

from conftest import GOLDEN


def _rocrand_table(name, index):
    t = json.load(open(os.path.join(GOLDEN, "rocrand_xorwow_tables.json")))["tables"]
    return np.array(t[name][str(index)], dtype=np.uint32).reshape(160, 5)


def test_jump_matrix_matches_rocrand(oracle):
    # rocRAND: sequence_jump_matrices[k] = A^(4^k * 2^67) (rocrand_xorwow.h:183-190); ours: A^(2^k * 2^67)
    assert np.array_equal(oracle.xorwow_matrix(0), _rocrand_table("h_xorwow_sequence_jump_matrices", 0))
    assert np.array_equal(oracle.xorwow_matrix(2), _rocrand_table("h_xorwow_sequence_jump_matrices", 1))
    assert np.array_equal(oracle.xorwow_matrix(12), _rocrand_table("h_xorwow_sequence_jump_matrices", 6))
    # and the one-step matrix is rocRAND's jump_matrices[0] = A^1
    assert np.array_equal(oracle.xorwow_matrix(-1), _rocrand_table("h_xorwow_jump_matrices", 0))


def test_step_is_linear_and_matches_matrix(oracle):
    rng = np.random.default_rng(1)
    A = oracle.xorwow_matrix(-1)
    for _ in range(20):
        st = np.concatenate([rng.integers(0, 2**32, 5, dtype=np.uint64).astype(np.uint32), np.zeros(1, np.uint32)])
        v = st[:5].copy()
        oracle.xorwow_next(st, 1)
        r = np.zeros(5, np.uint32)
        for b in range(160):
            if (int(v[b // 32]) >> (b % 32)) & 1:
                r ^= A[b]
        assert np.array_equal(r, st[:5]) and st[5] == 362437


def test_subsequence_composition(oracle):
    # jumping to subsequence a+b == jump a then jump b (powers of one matrix commute)
    s5 = oracle.xorwow_init(103033, 5)
    M0, M2 = oracle.xorwow_matrix(0), oracle.xorwow_matrix(2)
    v = oracle.xorwow_init(103033, 0)[:5]
    for M in (M0, M2):
        r = np.zeros(5, np.uint32)
        for b in range(160):
            if (int(v[b // 32]) >> (b % 32)) & 1:
                r ^= M[b]
        v = r
    assert np.array_equal(v, s5[:5])
    assert s5[5] == oracle.xorwow_init(103033, 0)[5]          # d is untouched by subsequence skips


def test_seed_scramble_constants(oracle):
    seed = 103033
    s0 = (seed & 0xFFFFFFFF) ^ 0xAAD26B49; s1 = (seed >> 32) ^ 0xF7DCEFDD
    t0 = (1099087573 * s0) & 0xFFFFFFFF; t1 = (2591861531 * s1) & 0xFFFFFFFF
    exp = [(123456789 + t0) & 0xFFFFFFFF, 362436069 ^ t0, (521288629 + t1) & 0xFFFFFFFF, 88675123 ^ t1,
           (5783321 + t0) & 0xFFFFFFFF, (6615241 + t1 + t0) & 0xFFFFFFFF]
    assert [int(v) for v in oracle.xorwow_init(seed, 0)] == exp


def test_uniform_range_and_mapping(oracle):
    st = oracle.xorwow_init(103033, 7)
    st2 = st.copy()
    u = oracle.xorwow_next(st, 4096)
    f = oracle.xorwow_uniform(st2, 4096)
    assert f.min() > 0.0 and f.max() <= 1.0
    exp = (u.astype(np.float32) * np.float32(2.3283064e-10) + np.float32(1.1641532e-10)).astype(np.float32)
    assert np.array_equal(exp.view(np.uint32), f.view(np.uint32))
    assert abs(f.mean() - 0.5) < 0.02


def test_committed_kats(oracle):
    kat = json.load(open(os.path.join(GOLDEN, "xorwow_kat.json")))
    for sub, k in kat["streams"].items():
        st = oracle.xorwow_init(kat["seed"], int(sub))
        assert [int(v) for v in st] == k["state"]
        st2 = st.copy()
        assert [int(v) for v in oracle.xorwow_next(st, 8)] == k["u32"]
        assert [int(v) for v in oracle.xorwow_uniform(st2, 8).view(np.uint32)] == k["uniform_bits"]
