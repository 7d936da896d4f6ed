"""Float64 restatement of the sampling rule of csrc/sample.hip (include/mmfd.h mmfd_sample_select), starting from
the fp32 quotients s_i = logits_i / temperature: transformers' TemperatureLogitsWarper -> TopKLogitsWarper ->
TopPLogitsWarper (min_tokens_to_keep = 1), softmax, one draw; equal s ordered by the lower index; a NaN never kept.

TOL, the bound every comparison uses, in units of eps = 2^-24 (the relative error of one correctly rounded fp32
operation). The kernel's mass of entry i is the integer round(e_i * 2^40), e_i its fp32 value of exp(s_i - m):
  d = fl(s_i - m)                                   relative error eps in d, so |d| eps in e_i; an entry of non-zero
                                                    mass has d > -41 ln 2 = -28.42:                      <= 28.5 eps
  d log2(e) as t + lo (two-float product, FMA)      exact to ~2^-48 |t|:                                 negligible
  2^t by the hardware                               <= 1 ulp <= 2^-23:                                   <= 2 eps
  e (1 + lo ln 2) by one FMA                        one rounding (the dropped second-order term ~1e-11):  <= 1 eps
  rounding to an integer of 2^-40                   <= 2^-41 each, V of them against S >= 1:             V 2^-41
so every mass is within 31.5 eps of e_i relatively, and a sum of non-negative terms keeps the terms' relative error:
any prefix A and the totals S, S_k computed from integer masses (integer sums are exact) are within
(31.5 + V 2^-17) eps of the float64 values, relative to S — below 32 eps for V <= 65536, the largest row the tests use
being 32769. A ratio A / S, and the two sides of the draw's comparison prefix > u S_k, are then within 2 * 32 eps:
TOL = 64 * 2^-24. (A probability e_i / S_k carries (|d| + 3) eps from its own mass, weighted by p_i <= e^d, i.e. at
most (1/e + 3) eps, 32 eps from S_k and 2 eps from the fp32 reciprocal and product: < 38 eps < TOL.)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.dropout_hash import dropout_hash

TOL = 64 * 2.0 ** -24

# (temperature, top_k, top_p): the settings of the issue's case table
SETTINGS = [(1.0, 0, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.9), (1.3, 50, 1.0), (0.7, 0, 0.5), (1.0, 5, 0.95), (1.0, 1, 1.0),
            (1.0, 0, 0.0)]
VOCABS = [1, 7, 200, 1001, 30524]
SIGMAS = [1.0, 1.5, 2.0, 3.0]
RESIDENT_MAX = 32768  # mmfd_sample_select_resident_max(): the tests take one V on each side (and check the query)
TEST_VOCABS = VOCABS + [RESIDENT_MAX, RESIDENT_MAX + 1]
MAX_ROWS = 32
# Row `seed` of a (V, setting) case is make_logits(V, seed). A row is usable when no survivor's A_i / S lies within
# 2 TOL of top_p (filter_ref's gap): only then must the kept sets be equal. A case of R rows uses the first R seeds
# of its list: 0 .. 31, except for the cases below, whose lists are the first 32 usable seeds counting up from 0
# (a 0.9 nucleus over 30,000 N(0, 1) logits steps by about 1e-5 per entry at its boundary, which is 2 TOL: most
# of those rows are not usable). test_sample_ref_cpu.py asserts that every seed of every list is usable.
SEEDS = {
    (1001, 1): [s for s in range(33) if s != 18],
    (30524, 1): [6, 7, 11, 15, 19, 31, 39, 43, 54, 55, 58, 59, 63, 66, 67, 71, 74, 82, 83, 87, 95, 99, 103, 107, 111, 114,
                 115, 119, 123, 127, 131, 138],
    (30524, 4): [s for s in range(33) if s != 24],
    (32768, 1): [3, 7, 11, 14, 15, 19, 27, 30, 31, 35, 43, 50, 54, 55, 59, 63, 66, 67, 71, 75, 79, 86, 87, 91, 99, 103,
                 106, 107, 111, 118, 119, 123],
    (32769, 1): [3, 6, 7, 11, 19, 27, 30, 31, 39, 47, 51, 54, 55, 59, 66, 67, 75, 79, 83, 91, 95, 99, 107, 111, 127, 131,
                 135, 139, 147, 151, 158, 159],
    (32769, 4): [s for s in range(33) if s != 24],
}


def make_logits(V, seed):
    """the row of seed `seed`: N(0, sigma^2) logits, sigma by the seed"""
    rng = np.random.default_rng([int(seed), int(V)])
    return (rng.standard_normal(V) * SIGMAS[seed % 4]).astype(np.float32)


def case_seeds(V, si, R=MAX_ROWS):
    return SEEDS.get((V, si), list(range(MAX_ROWS)))[:R]


def case_logits(V, si, R):
    """[R, V] fp32 logits of the (V, setting) case: its first R usable seeds"""
    return np.stack([make_logits(V, s) for s in case_seeds(V, si, R)])


def quotients(logits, temperature):
    """s = logits / temperature, one correctly rounded fp32 division"""
    return (np.asarray(logits, np.float32) / np.float32(temperature)).astype(np.float32)


@dataclass
class Filtered:
    kept: np.ndarray      # bool [V]
    mass: np.ndarray      # float64 [V]: exp(s - m) of the kept entries, 0 elsewhere
    probs: np.ndarray     # float64 [V]: mass / S_k
    a_over_s: np.ndarray  # float64 [V]: A_i / S of the top-k survivors (nan elsewhere)
    gap: float            # min |A_i / S - top_p| over the survivors after the first (inf without a nucleus filter)
    n_kept: int


def filter_ref(s, top_k, top_p):
    s = np.asarray(s, np.float32)
    V = s.shape[0]
    number = ~np.isnan(s) & (s > -np.inf)
    kept = np.zeros(V, bool)
    nan = np.full(V, np.nan)
    if not number.any():
        return Filtered(kept, np.zeros(V), np.zeros(V), nan, np.inf, 0)
    v = np.where(np.isnan(s), -np.inf, s).astype(np.float64)
    surv = number.copy()
    if 0 < top_k < V:
        tau = np.sort(v)[V - top_k]  # the top_k-th largest, duplicates counted (a NaN below every number)
        surv &= v >= tau
    idx = np.nonzero(surv)[0]
    m = v[idx].max()
    with np.errstate(invalid="ignore"):
        e = np.where(v[idx] == m, 1.0, np.exp(v[idx] - m))
    e = np.where(np.isnan(e), 0.0, e)
    S = e.sum()
    a_over_s, gap = nan.copy(), np.inf
    if np.float32(top_p) < 1:
        order = np.argsort(-v[idx], kind="stable")  # larger s first, equal s by the lower index
        A = np.cumsum(e[order]) - e[order]
        keep_o = A < float(np.float32(top_p)) * S
        keep_o[0] = True
        a_over_s[idx[order]] = A / S
        if len(order) > 1:
            gap = float(np.abs(A[1:] / S - float(np.float32(top_p))).min())
        kept[idx[order[keep_o]]] = True
    else:
        a_over_s[idx] = 0.0
        kept[idx] = True
    mass = np.zeros(V)
    mass[idx] = e
    mass[~kept] = 0.0
    return Filtered(kept, mass, mass / mass.sum(), a_over_s, gap, int(kept.sum()))


def usable(f: Filtered):
    return f.gap >= 2 * TOL


def uniform_ref(seed, step, row):
    """u of (seed, step, row): the top 24 bits of mmfd_hash(seed, salt = step, idx = row) on the 2^-24 grid"""
    return float(int(dropout_hash(int(seed), int(step), np.uint64(row))) >> 8) * 2.0 ** -24


def draw_ref(f: Filtered):
    """the inclusive prefix table C_j / S_k in index order"""
    return np.cumsum(f.probs)


def accepted(f: Filtered, token, u, widen=0.0):
    """C_{j-1} - TOL S_k <= u S_k < C_j + TOL S_k for j = token (in units of S_k)"""
    j = int(token)
    if not 0 <= j < f.kept.shape[0]:
        return False
    C = draw_ref(f)
    before = C[j - 1] if j > 0 else 0.0
    tol = TOL + widen
    return bool(before - tol <= u < C[j] + tol)


def hf_kept(logits, temperature, top_k, top_p):
    """the kept set of transformers' three warpers, in BLIP's order"""
    import torch
    from transformers.generation.logits_process import (TemperatureLogitsWarper, TopKLogitsWarper,
                                                         TopPLogitsWarper)
    x = torch.from_numpy(np.asarray(logits, np.float32))[None]
    ids = torch.zeros(1, 1, dtype=torch.long)
    if temperature != 1.0:
        x = TemperatureLogitsWarper(float(temperature))(ids, x)
    if top_k > 0:
        x = TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=1)(ids, x)
    if top_p < 1.0:
        x = TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=1)(ids, x)
    return torch.isfinite(x[0]).numpy()
