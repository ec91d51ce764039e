"""Integer model of ONE pass of the second-generation NTT (csrc/ntt_pass.hip) and the input families its stage tests run (TEST INFRASTRUCTURE ONLY).

Plain Python integers; imports nothing from the product.  The model works on the integers the buffers HOLD -- the Montgomery words x 2^256 mod r read
as integers mod r -- because every step of a pass is linear in them: a butterfly is (a + b, (a - b) w), the scales are field constants.  So a word that
is congruent to the model's integer is right, whatever representative a scratch format stores.

  pass_plan(n)          the stage bits of a 2^n transform split into passes, restated from its definition (ntt_pass.h)
  run_pass(...)         one pass: stage bits [s_lo, s_lo + K), high to low, with the first-pass and last-pass rules
  encode / decode       the three scratch formats and the canonical element, as u32 words
  FAMILIES              named input builders, each a function of (n, s_lo, K, seed, top)
"""
from __future__ import annotations

import random

import numpy as np

R = 8444461749428370424248824938781546531375899335154063827935233455917409239041
GENERATOR = 22                 # the coset shift g
TWO_ADICITY = 47
MONT = (1 << 256) % R          # the Montgomery one: stored word of the field element 1
# LARGE_SUBGROUP_ROOT_OF_UNITY as the parameter file stores it (a Montgomery word); its cube is the 2^47-th root the radix-2 domains square down from
_LARGE_SUBGROUP_ROOT_WORD = 0x0C59F8D8D6F0DC97_3FBBB698ADABCF93_7175A69E39013BFF_9BFE9D90C790C167
SENTINEL_WORD = 0xA5A5A5A5
DEADBEEF = sum(0xDEADBEEFDEADBEEF << (64 * i) for i in range(4))   # the tail behind in_len: not canonical, must not be read

# (B0, RB, KB) of every step of a pass over K stage bits, KB for canonical inputs (times 2 for scratch inputs < 2 r): the row bits [B0, B0 + RB) a
# step owns and the bound constant its radix-8 (RB = 3) or radix-4 (RB = 2) groups are instantiated with.  NTT_CHAINS is the same table by kind.
STEPS = {7: [(4, 3, 2), (2, 2, 16), (0, 2, 64)], 6: [(3, 3, 2), (0, 3, 16)], 5: [(2, 3, 2), (0, 2, 16)]}
NTT_CHAINS = {K: [("radix8" if rb == 3 else "radix4", kb) for _, rb, kb in steps] for K, steps in STEPS.items()}


def root_of_unity(n):
    """the generator of the 2^n domain as a plain integer: LARGE^3 squared 47 - n times"""
    assert 0 <= n <= TWO_ADICITY
    w = pow(_LARGE_SUBGROUP_ROOT_WORD * pow(1 << 256, -1, R) % R, 3, R)
    for _ in range(TWO_ADICITY - n):
        w = w * w % R
    return w


def omega(n, inverse=False):
    w = root_of_unity(n)
    return pow(w, -1, R) if inverse else w


def pass_plan(n):
    """[(K, s_lo)] per pass: the n stage bits in ceil(n / 7) near-equal groups, the larger ones first, highest bits first; n = 0 is one empty pass"""
    m = 1 if n == 0 else (n + 6) // 7
    out, s = [], n
    for p in range(m):
        k = n // m + (1 if p < n % m else 0)
        s -= k
        out.append((k, s))
    return out


def equal_groups(n):
    m = len(pass_plan(n))
    return m >= 2 and n % m == 0


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def run_pass(values, n, s_lo, K, omega, first=False, in_len=None, prescale=False, last=False, post_mode=0, addend=None, c2=None):
    """One pass over the stage bits [s_lo, s_lo + K) of a 2^n transform with the root `omega`.
    first: elements >= in_len read as 0 (`values` may be shorter than 2^n, and what it holds behind in_len is not looked at); with prescale element i
    is multiplied by g^i first.  last (s_lo = 0): output index = the n-bit reversal of the input index, then the post mode at OUTPUT index k:
    1  * 1/D;  2  * g^-k / D;  3  (v g^-k / D - addend_k) * c2;  4  v + addend_k.  Returns 2^n integers in [0, r)."""
    D = 1 << n
    assert s_lo + K <= n and (not last or s_lo == 0)
    if first:
        in_len = D if in_len is None else in_len
        v = [values[i] % R if i < in_len else 0 for i in range(D)]
        if prescale:
            g = 1
            for i in range(D):
                v[i] = v[i] * g % R
                g = g * GENERATOR % R
    else:
        assert len(values) == D and not prescale
        v = [x % R for x in values]
    pw = [1] * D
    for j in range(1, D):
        pw[j] = pw[j - 1] * omega % R
    for q in range(K - 1, -1, -1):
        s = s_lo + q
        half, step = 1 << s, D >> (s + 1)            # w_s = omega^(D >> (s + 1)), exponent i mod 2^s
        for blk in range(0, D, 2 * half):
            for j in range(half):
                i = blk + j
                a, b = v[i], v[i + half]
                v[i] = (a + b) % R
                v[i + half] = (a - b) * pw[step * j] % R
    if not last:
        assert post_mode == 0
        return v
    out = [0] * D
    for i in range(D):
        out[bitrev(i, n)] = v[i]
    dinv, ginv = pow(D, -1, R), pow(GENERATOR, -1, R)
    if post_mode == 1:
        out = [x * dinv % R for x in out]
    elif post_mode in (2, 3):
        t = dinv
        for k in range(D):
            out[k] = out[k] * t % R
            t = t * ginv % R
        if post_mode == 3:
            out = [(x - addend[k]) * c2 % R for k, x in enumerate(out)]
    elif post_mode == 4:
        out = [(x + addend[k]) % R for k, x in enumerate(out)]
    else:
        assert post_mode == 0
    return out


def run_fused(values, n, C):
    """the fused pass of an ifft -> coset_fft pair: the inverse transform's last pass (bits [0, C), 1 / D), then the forward transform's first pass
    (g^i, bits [n - C, n))"""
    mid = run_pass(values, n, 0, C, omega(n, True), last=True, post_mode=1)
    return run_pass(mid, n, n - C, C, omega(n), first=True, prescale=True)


def transform(values, n, kind, in_len=None):
    """the model composed over pass_plan(n).  kind: 0 fft, 1 ifft, 2 coset_fft, 3 coset_ifft (the ABI's numbering)"""
    inverse = kind in (1, 3)
    plan = pass_plan(n)
    v = values
    for p, (K, s_lo) in enumerate(plan):
        v = run_pass(v, n, s_lo, K, omega(n, inverse), first=p == 0, in_len=in_len if p == 0 else None, prescale=p == 0 and kind == 2,
                     last=p + 1 == len(plan), post_mode=(0, 1, 0, 2)[kind] if p + 1 == len(plan) else 0)
    return v


# ------------------------------------------------------------------------------------------------------------------------ codecs
# format 0: canonical 8 x u32 (< r);  1: nine normalised 29-bit limbs, value < 2 r;  2: value < 2 r in 8 x u32.  "canon" = format 0.
def words_per_elem(fmt):
    return 9 if fmt == 1 else 8


def encode(values, fmt, check=True):
    """integers -> (len, words) u32.  check=False writes the words of any integer below 2^256 (2^261 for format 1): the not-to-be-read tails"""
    if check:
        bound = R if fmt == 0 else 2 * R
        assert all(0 <= v < bound for v in values), "value outside the format's range"
    if fmt == 1:
        return np.array([[(v >> (29 * i)) & ((1 << 29) - 1) if i < 8 else v >> 232 for i in range(9)] for v in values], dtype=np.uint32).reshape(len(values), 9)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint32).reshape(len(values), 8).copy()


def decode(rows, fmt):
    """(len, words) u32 -> integers, raw: the caller checks ranges (in_range) -- a sentinel row decodes to a value outside every range"""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    if fmt == 1:
        return [sum(int(x) << (29 * i) for i, x in enumerate(r)) for r in rows]
    raw = rows.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(rows.shape[0])]


def in_range(rows, values, fmt):
    """what a format promises of element words: the value bound, and for format 1 normalised limbs"""
    bound = R if fmt == 0 else 2 * R
    ok = all(v < bound for v in values)
    if fmt == 1:
        ok = ok and bool((np.asarray(rows) < (1 << 29)).all())
    return ok


# ------------------------------------------------------------------------------------------------------------------------ families
def _const(c):
    return lambda n, s_lo, K, seed, top: [c(top) if callable(c) else c] * (1 << n)


def _stage(q, swap):
    def f(n, s_lo, K, seed, top):
        assert q < K
        return [top if ((i >> (s_lo + q)) & 1) == (1 if swap else 0) else 0 for i in range(1 << n)]
    return f


def _impulse(where):
    def f(n, s_lo, K, seed, top):
        D = 1 << n
        v = [0] * D
        v[{"0": 0, "1": 1, "half": D // 2, "last": D - 1}[where]] = top
        return v
    return f


def _random(n, s_lo, K, seed, top):
    rng = random.Random(seed)
    return [rng.randint(0, top) for _ in range(1 << n)]


def alias_pair(n, seed):
    """scratch only: a random canonical vector a and its alias a' = a + r on a random half of the elements (both < 2 r)"""
    rng = random.Random(seed)
    a = [rng.randrange(R) for _ in range(1 << n)]
    return a, [x + R if rng.getrandbits(1) else x for x in a]


def families(K, scratch):
    """name -> builder(n, s_lo, K, seed, top), top = r - 1 for canonical inputs and 2 r - 1 for scratch inputs"""
    f = {"all_top": _const(lambda top: top), "all_0": _const(0), "all_1": _const(1)}
    if scratch:
        f["all_r"] = _const(R)
    for q in range(K):
        f["stage%d_low" % q] = _stage(q, False)      # top where bit s_lo + q of the index is 0, 0 elsewhere
        f["stage%d_high" % q] = _stage(q, True)      # the swap
    for where in ("0", "1", "half", "last"):
        f["impulse_" + where] = _impulse(where)
    f["random"] = _random
    return f


def top_of(scratch):
    return 2 * R - 1 if scratch else R - 1


def prefix_lengths(n):
    D = 1 << n
    return [0, 1, D // 2 + 1, D - 3, D]


def prefix_input(n, in_len, stride, seed):
    """first passes: `stride` integers, random canonical below in_len, DEADBEEF behind it"""
    rng = random.Random(seed)
    assert in_len <= stride
    return [rng.randrange(R) if i < in_len else DEADBEEF for i in range(stride)]
