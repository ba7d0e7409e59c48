"""Cases and Python-integer expectations for the scalar layer (narwhal_amd/csrc/nw_scalar.hpp)
and the scalar phase of a strict verification (nw_strict.hpp strict_scalar_phase, bdigits,
key_recode / key_digit), as tools/sc_ops.hpp dispatches them. tests/test_sc_ops_cpu.py runs the
batches on the CPU build (tools/libnw_hostcheck.so hc_sc_ops), tests/test_gpu_sc_ops.py on the
gfx950 build (tools/libnw_lpcheck.so k_sc_ops). Nothing here uses project code: the
expectations are Python integers, an exact Euclidean algorithm and a word-level model of the
Barrett step that only CLASSIFIES inputs (how many final subtractions, whether the 9-word
difference wraps), so that the tests can assert that their inputs reach what they claim.

A case is 24 input words, one integer k and 40 output words (tools/sc_ops.hpp)."""
import random

import numpy as np

# ---- operation codes (tools/sc_ops.hpp sc_op_code) ------------------------------------------
(REDUCE512, MUL, ADD, NEG, CANONICAL, RECODE, HALF_SPLIT, HALF_SPLIT_ONESTEP, SCALAR_PHASE_16,
 SCALAR_PHASE_24, BDIGITS_8, BDIGITS_16, BDIGITS_20, BDIGITS_24, KEY_DIGITS, SC_N) = range(16)
IN_WORDS, OUT_WORDS = 24, 40

L = 2**252 + 27742317777372353535851937790883648493
N8 = 8 * L                 # the group order: the half-size split's lattice is mod 8l
B9 = 2**288
MU = 2**512 // L           # Barrett's mu for b = 2^32, k = 8
ITER_CAP = 400             # sc_half_split's iteration cap (the code's own constant)
QCAP = 2**32 - 1           # the largest quotient one one-step iteration takes
COST_EXACT = 100           # cost <= this: the result is exact (a factor of 4 below the cap for
                           # f64 underestimates and iterations a lane waits on its wave)


def words(x, n):
    assert 0 <= x < 2**(32 * n)
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def val(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def i32(w):
    return w - 2**32 if w >= 2**31 else w


class Batch:
    """Cases of one operation code: (name, input words, k, check, exact). check(out words)
    asserts; exact: the two builds must agree word for word on this case."""

    def __init__(self, op):
        self.op, self.cases = op, []

    def add(self, name, inp, k, check, exact=True):
        assert len(inp) <= IN_WORDS
        self.cases.append((name, list(inp), k, check, exact))

    def arrays(self):
        n = len(self.cases)
        A = np.zeros((n, IN_WORDS), np.uint32)
        for i, c in enumerate(self.cases):
            A[i, :len(c[1])] = c[1]
        return A, np.array([i32(c[2] & 0xffffffff) for c in self.cases], np.int32)

    def exact_rows(self):
        return np.array([c[4] for c in self.cases], bool)

    def check(self, out):
        assert len(out) == len(self.cases)
        for (name, _, _, chk, _), row in zip(self.cases, out.tolist()):
            try:
                chk(row)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None


def _is(expected, n=8):
    ws = words(expected, n)

    def chk(o):
        assert o[:n] == ws, ("got", hex(val(o[:n])), "want", hex(expected))
        assert not any(o[n:]), ("words past the result written", o[n:])
    return chk


# ---- Barrett: a word-level model that classifies an input -----------------------------------
def barrett(x):
    """HAC 14.42 with b = 2^32, k = 8 as sc_reduce512 runs it: (x mod l, final subtractions,
    whether x mod b^9 - q3 l mod b^9 wraps, whether row 0 of q3 * l carries into word 8)."""
    assert 0 <= x < 2**512
    q3 = ((x >> 224) * MU) >> 288
    r1, r2 = x % B9, (q3 * L) % B9
    r = (r1 - r2) % B9
    subs = 0
    while r >= L:
        r -= L
        subs += 1
    assert r == x % L
    return r, subs, r1 < r2, (((q3 & 0xffffffff) * L) >> 256) != 0


# q3 >= floor(x / l) - 1 for every x < 2^512, so two subtractions never happen: q3 =
# floor(x / l - e) with e = e1 + e2, e1 < 2^-28 lost by dropping x mod b^7 and e2 =
# frac(2^512 / l) * floor(x / b^7) / b^9 < frac(2^512 / l) lost by truncating mu; the
# inequality below is frac(2^512 / l) + 2^-28 < 1 in integers (the fraction is 0.2249...).
TWO_SUBTRACTIONS_IMPOSSIBLE = (2**512 % L) * 2**28 + L < L * 2**28


def search_two_subtractions(seed=5, tries=120000):
    """A bounded search for an input needing two final subtractions, aimed where the estimate
    loses most: x = q l + r with r small (a quotient one too small already costs r / l) and x's
    top words large (mu's truncation error grows with floor(x / b^7)). Returns the inputs
    found."""
    rng = random.Random(seed)
    qmax = (2**512 - 1) // L
    found = []
    for i in range(tries):
        if i % 3 == 0:
            x = rng.getrandbits(512)
        else:
            q = qmax - rng.getrandbits(rng.choice((8, 64, 200, 258)))
            x = min(q * L + rng.getrandbits(rng.choice((1, 32, 200))), 2**512 - 1)
        if barrett(x)[1] >= 2:
            found.append(x)
    return found


def reduce_inputs():
    """(name, x) for sc_reduce512: the listed values, q l + r over the quotient sizes, and inputs
    the model places in each class."""
    qmax = (2**512 - 1) // L
    xs = [("0", 0), ("1", 1), ("l-1", L - 1), ("l", L), ("l+1", L + 1), ("2l-1", 2 * L - 1),
          ("2l", 2 * L), ("2^252", 2**252), ("2^253-1", 2**253 - 1), ("2^256-1", 2**256 - 1),
          ("2^512-1", 2**512 - 1), ("qmax*l", qmax * L), ("qmax*l-1", qmax * L - 1),
          ("qmax*l+1", qmax * L + 1), ("15l+l-1", 16 * L - 1), ("b^9", B9), ("b^9-1", B9 - 1),
          ("l*2^259", L * 2**259)]
    rng = random.Random(21)
    for qb in (1, 64, 128, 200, 259):
        for q in (2**(qb - 1), 2**qb - 1, 2**(qb - 1) | rng.getrandbits(qb - 1)):
            for rn, r in (("0", 0), ("1", 1), ("l-1", L - 1)):
                if q * L + r < 2**512:
                    xs.append((f"q{qb}bits={q:#x},r={rn}", q * L + r))
    # the difference wraps where x mod b^9 is below the true difference (x mod l, plus l per
    # subtraction): a multiple of b^9 plus a little
    for i in range(48):
        m = rng.getrandbits(224)
        xs.append((f"wrap{i}", m * B9 + rng.getrandbits(rng.choice((0, 1, 64, 200, 250)))))
    for i in range(600):
        xs.append((f"rand{i}", rng.getrandbits(512)))
    for i in range(64):
        xs.append((f"small{i}", rng.getrandbits(rng.choice((8, 100, 255, 256, 257, 300)))))
    return xs


def mul_inputs():
    rng = random.Random(22)
    edge = [0, 1, 2, L - 1, L, L + 1, 2 * L - 1, 2**252, 2**253 - 1, 2**255, 2**256 - 1,
            2**256 - 2**224, 2**128 - 1, 2**128, 0xffffffff, 2**32]
    ps = [(f"edge{a:#x}*{b:#x}", a, b) for a in edge for b in edge]
    for i in range(200):
        ps.append((f"rand{i}", rng.getrandbits(256), rng.getrandbits(256)))
    for i in range(100):   # verify_batch's z k, the scalar phase's |v| s
        ps.append((f"z128*k{i}", rng.getrandbits(128) | 2**127, rng.randrange(L)))
        ps.append((f"v160*s{i}", rng.getrandbits(160) | 2**159, rng.randrange(L)))
        ps.append((f"v128*s{i}", rng.getrandbits(128) | 1, rng.randrange(L)))
    for s in (0, 1, L - 1):
        ps.append((f"v160max*{s:#x}", 2**160 - 1, s))
    return ps


def _g_barrett():
    red = Batch(REDUCE512)
    for name, x in reduce_inputs():
        red.add(name, words(x, 16), 0, _is(x % L))
    mul = Batch(MUL)
    for name, a, b in mul_inputs():
        mul.add(name, words(a, 8) + words(b, 8), 0, _is(a * b % L))
    return [red, mul]


def _g_addneg():
    rng = random.Random(23)
    add = Batch(ADD)
    pairs = []
    for tot in (L - 1, L, L + 1, 2 * L - 2):
        for a in (L - 1, (tot + 1) // 2, rng.randrange(max(0, tot - L + 1), min(L, tot + 1)),
                  tot - (L - 1), 2**252):
            if 0 <= a < L and 0 <= tot - a < L:
                pairs.append((a, tot - a))
    pairs += [(0, 0), (0, L - 1), (1, L - 1), (L - 1, L - 1), (2**252 - 1, 1), (2**224 - 1, 1)]
    pairs += [(rng.randrange(L), rng.randrange(L)) for _ in range(300)]
    for tot in (L - 1, L, L + 1, 2 * L - 2):
        assert any(a + b == tot for a, b in pairs)
    for a, b in pairs:
        add.add(f"{a:#x}+{b:#x}", words(a, 8) + words(b, 8), 0, _is((a + b) % L))
        add.add(f"{b:#x}+{a:#x}", words(b, 8) + words(a, 8), 0, _is((a + b) % L))
    neg = Batch(NEG)
    for a in [0, 1, 2, L - 1, L - 2, 2**252, 2**252 - 1, 2**32, 2**32 - 1, L - 2**32,
              L % 2**128, L % 2**128 + 1, L % 2**128 - 1] + [rng.randrange(L) for _ in range(200)]:
        neg.add(f"-{a:#x}", words(a, 8), 0, _is((L - a) % L))
    can = Batch(CANONICAL)
    vs = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2**252, 2**252 - 1, 2**253 - 1, 2**253,
          2**255, 2**256 - 1, L % 2**128, 2**252 + 2**128]
    for i in range(8):   # l with one word one up / one down: each word decides once
        vs += [L + 2**(32 * i), L - 2**(32 * i)]
    vs += [rng.getrandbits(256) for _ in range(100)] + [rng.randrange(L) for _ in range(100)]
    for v in vs:
        can.add(f"{v:#x}", words(v, 8), 0, _is(1 if v < L else 0, 1))
    return [add, neg, can]


# ---- signed-digit recodings -----------------------------------------------------------------
def bdigit_spec(bw):
    """bdigits<BW> / keyspec_for(W): (digits, signed digits, bias)."""
    nb = (253 + bw - 1) // bw
    nsigned = nb - 1 if nb * bw > 256 else nb
    return nb, nsigned, sum(2**(bw * m + bw - 1) for m in range(nsigned))


def recode_values(bw, limit=2**253):
    nd = (256 + bw - 1) // bw
    vs = [("0", 0), ("1", 1), ("l-1", L - 1), ("l", L), ("2^253-1", 2**253 - 1),
          ("2^252-1", 2**252 - 1), ("2^252", 2**252)]
    half = 2**(bw - 1)
    for d in (half - 1, half, half + 1, 2**bw - 1):
        vs.append((f"every digit {d:#x}", sum(d << (bw * m) for m in range(nd)) % 2**253))
        vs.append((f"digit 0 zero, others {d:#x}", sum(d << (bw * m) for m in range(1, nd)) % 2**253))
        vs.append((f"only digit 0 {d:#x}", d))
    rng = random.Random(30 + bw)
    vs += [(f"rand{i}", rng.randrange(L)) for i in range(64)]
    return [(n, v % limit) for n, v in vs]


def _digits_check(w, bw):
    nb, nsigned, bias = bdigit_spec(bw)

    def chk(o):
        assert val(o[:8]) == w + bias, ("recoded words", hex(val(o[:8])))
        ds = [i32(x) for x in o[8:8 + nb]]
        assert not any(o[8 + nb:])
        assert sum(d << (bw * m) for m, d in enumerate(ds)) == w, ("digits", ds)
        for m, d in enumerate(ds):
            if m < nsigned:
                assert -2**(bw - 1) <= d < 2**(bw - 1), (m, d)
            else:
                assert 0 <= d, ("the top digit is unsigned", d)
            assert abs(d) <= 2**(bw - 1), ("past the table's last entry", m, d)
    return chk


def _g_recode():
    out = []
    for bw, word in ((4, 0x88888888), (8, 0x80808080)):
        b = Batch(RECODE)
        bias = val([word] * 8)
        for name, s in recode_values(bw):
            def chk(o, s=s, bw=bw, bias=bias):
                assert val(o[:8]) == s + bias and not any(o[8:])
                ds = [((val(o[:8]) >> (bw * m)) & (2**bw - 1)) - 2**(bw - 1) for m in range(256 // bw)]
                assert sum(d << (bw * m) for m, d in enumerate(ds)) == s
            b.add(f"bias {word:#x}: {name}", words(s, 8), word, chk)
        out.append(b)
    for bw, op in ((8, BDIGITS_8), (16, BDIGITS_16), (20, BDIGITS_20), (24, BDIGITS_24)):
        b = Batch(op)
        kd = Batch(KEY_DIGITS)
        for name, w in recode_values(bw):
            b.add(f"bdigits<{bw}>: {name}", words(w, 8), 0, _digits_check(w, bw))
            kd.add(f"key digits W={bw}: {name}", words(w, 8), bw, _digits_check(w, bw))
        out += [b, kd]
    return out


# ---- the half-size split --------------------------------------------------------------------
def euclid(k):
    """Exact Euclid on (8l, k) down to the first remainder below 2^128: the quotients, then
    X = (previous remainder, its cofactor) and Y = (that remainder, its cofactor), r = t k
    (mod 8l)."""
    r0, r1, t0, t1 = N8, k, 0, 1
    qs = []
    while r1 >= 2**128:
        q = r0 // r1
        qs.append(q)
        r0, r1 = r1, r0 - q * r1
        t0, t1 = t1, t0 - q * t1
    return qs, (r0, t0), (r1, t1)


def band(qs):
    """"low": the one-step loop needs at most COST_EXACT iterations, the result is determined;
    "high": the quotients >= 2^32 alone need more than the cap, the result is the fallback;
    "mid": only the invariants apply (and the two builds, or two waves, may differ)."""
    if sum(-(-q // QCAP) for q in qs) <= COST_EXACT:
        return "low"
    if sum(q >> 32 for q in qs if q >= 2**32) > ITER_CAP:
        return "high"
    return "mid"


def onestep_exact(qs):
    """sc_half_split<false> has no Lehmer rounds and asks nothing of its wave, so its iteration
    count is its own: a quotient q takes at most ceil(q / (2^32 - 1)) + 2 iterations (the f64
    estimate floor(ratio (1 - 2^-46)) of a remaining quotient below 2^32 is at most 1 short, so
    after the capped steps one estimated step and one of q = 1 finish it). Within the cap the
    result is determined on every build, whatever band() says."""
    return sum(-(-q // QCAP) + 2 for q in qs) <= ITER_CAP


def _measure(r, t):
    return max(abs(r).bit_length(), abs(t).bit_length())


def half_expect(k, onestep=False):
    """(band, "odd" / "even" cofactor, check(u, |v|, vneg)); onestep: for sc_half_split<false>,
    whose band is "low" also where onestep_exact holds."""
    qs, (xr, xt), (yr, yt) = euclid(k)
    bnd, parity = band(qs), "odd" if yt % 2 else "even"
    if onestep and onestep_exact(qs):
        bnd = "low"

    def chk(u, av, neg):
        assert neg in (0, 1)
        v = -av if neg else av
        assert (u - v * k) % N8 == 0, ("u != v k (mod 8l)", hex(u), v)
        assert av % 2 == 1, ("v is even", v)
        assert 0 <= u < 2**253 and av < 2**160
        fallback = (u, av, neg) == (k, 1, 0)
        assert u < 2**252 or fallback, ("u >= 2^252 outside the fallback", hex(u))
        if bnd == "high":
            assert fallback, ("a quotient sum past the cap did not fall back", hex(u), v)
        if bnd == "low" and parity == "odd":
            assert (u, v) == (yr, yt), ("not the first remainder below 2^128", hex(u), v, hex(yr), yt)
            assert u < 2**128 and av < 2**128
        if bnd == "low" and parity == "even":
            bound = min(_measure(xr - yr, xt - yt), _measure(xr + yr, xt + yt))
            if fallback:
                assert bound >= 252, ("fallback although X -+ Y is short", bound)
            else:
                assert _measure(u, av) <= bound, ("longer than X -+ Y", _measure(u, av), bound)
    return bnd, parity, chk


LISTED_K = [(N8 * (2**126 + 1)) // (2**128 + 3) % L, N8 // (2**127 + 1) % L, 2**128 - 1, 2**128,
            2**252, L - 1, 0, 1, 2, 7, 2**129 + 5, 3 * 2**127, 2**200 + 1, N8 // 3 % L]

BIG_Q = [("2^31-1", 2**31 - 1), ("2^31+5", 2**31 + 5), ("2^32-1", 2**32 - 1), ("2^32", 2**32),
         ("2^32+7", 2**32 + 7), ("3*2^32+1", 3 * 2**32 + 1), ("100*2^32+3", 100 * 2**32 + 3),
         ("2^40", 2**40), ("2^45", 2**45)]
DEPTHS = (0, 1, 5, 20, 50)   # 20: a Lehmer round or two deep; 50: close to the stopping point


def _from_cf(terms):
    num, den = terms[-1], 1
    for a in reversed(terms[:-1]):
        num, den = a * num + den, num
    return N8 * den // num   # floor(8l / [a1; a2, ...])


_constructed = None


def constructed_k():
    """{(depth, quotient name): k}: 8l / k's continued fraction has `depth` small quotients,
    then the named one (confirmed with the exact Euclid), then small ones again."""
    global _constructed
    if _constructed is None:
        rng = random.Random(40)
        _constructed = {}
        for d in DEPTHS:
            for qn, Q in BIG_Q:
                prefix = [rng.choice((1, 1, 1, 2, 2, 3, 4, 6)) for _ in range(d)]
                if d:
                    prefix[0] = rng.randint(8, 40)   # k < l
                tail = [rng.choice((1, 1, 2, 3, 5)) for _ in range(40)]
                k = _from_cf(prefix + [Q] + tail)
                qs = euclid(k)[0]
                assert 0 < k < L and qs[:d] == prefix and qs[d] == Q, (d, qn)
                assert all(q < 2**31 - 1 for i, q in enumerate(qs) if i != d)
                _constructed[(d, qn)] = k
    return _constructed


_half = None


def half_k():
    """[(name, k)]: 2,000 seeded random k < l, the listed k, the constructed k."""
    global _half
    if _half is None:
        rng = random.Random(41)
        _half = [(f"rand{i}", rng.randrange(L)) for i in range(2000)]
        _half += [(f"listed{i}", k) for i, k in enumerate(LISTED_K)]
        _half += [(f"depth {d}, q={qn}", k) for (d, qn), k in constructed_k().items()]
        _half += [(f"early{b}", rng.getrandbits(b) | 2**(b - 1)) for b in (1, 64, 100, 127, 128)]
        # regression: one step to the remainder 8 with the even cofactor -8, every candidate has
        # u >= 2^252, so the result is the fallback. The gfx950 build of strict_scalar_phase
        # once returned X - Y's u = l - 9 beside the fallback's v = 1 (u != v k mod 8l)
        _half += [("regression k=l-1: even cofactor, fallback", L - 1),
                  ("regression k=l-2: even cofactor, fallback", L - 2)]
        # past COST_EXACT but inside onestep_exact: the one-step loop must still finish (with a
        # quotient cap of half the size it would not)
        _half += [(f"depth 0, q={m}*2^32+9", _from_cf([m * 2**32 + 9] + [1, 2, 1, 3] * 10))
                  for m in (150, 200)]
    return _half


def _half_check(k, onestep=False):
    bnd, _, chk = half_expect(k, onestep)

    def c(o):
        chk(val(o[:8]), val(o[8:13]), o[13])
        assert not any(o[14:])
    return c, bnd


def _g_half():
    out = []
    for op in (HALF_SPLIT, HALF_SPLIT_ONESTEP):
        b = Batch(op)
        for name, k in half_k():
            chk, bnd = _half_check(k, op == HALF_SPLIT_ONESTEP)
            b.add(name, words(k, 8), 0, chk, exact=bnd != "mid")
        out.append(b)
    return out


# ---- the scalar phase -----------------------------------------------------------------------
BIAS4_64 = val([0x88888888] * 8)
BIAS4_40 = val([0x88888888] * 5)


def _phase_check(k, s, bw):
    _, _, half = half_expect(k)
    bias = bdigit_spec(bw)[2]

    def chk(o):
        dig, vneg, W = o[:21], o[21], o[22]
        assert not any(o[23:])
        u, av, w = val(dig[:8]) - BIAS4_64, val(dig[8:13]) - BIAS4_40, val(dig[13:21]) - bias
        assert u >= 0 and av >= 0, "a recoding lost its carry"
        half(u, av, vneg)
        v = -av if vneg else av
        assert 0 <= w < L and w == (-v * s) % L, ("w != -v s mod l", hex(w))
        nib = [((val(dig[:8]) >> (4 * j)) & 15) - 8 for j in range(64)]
        nib_v = [((val(dig[8:13]) >> (4 * j)) & 15) - 8 for j in range(40)]
        assert sum(d << (4 * j) for j, d in enumerate(nib)) == u
        assert sum(d << (4 * j) for j, d in enumerate(nib_v)) == av
        top = max([j for j, d in enumerate(nib) if d] + [j for j, d in enumerate(nib_v) if d] + [-1])
        assert W == max(32, top + 1) and W <= 64, ("W", W, "highest nonzero digit", top)
        assert not any(nib[W:]) and not any(nib_v[W:])
    return chk


def phase_pairs():
    rng = random.Random(42)
    ks = half_k()
    chosen = [kk for kk in ks if not kk[0].startswith("rand")] + ks[:150]
    pairs = []
    for name, k in chosen:
        fixed = name.startswith("rand")
        ss = [("rand", rng.randrange(L))]
        if not fixed:
            ss += [("0", 0), ("1", 1), ("l-1", L - 1), ("bit252", 2**252 + rng.randrange(L - 2**252)),
                   ("2^252", 2**252)]
        pairs += [(f"k {name}, s {sn}", k, s) for sn, s in ss]
    return pairs


def _g_phase():
    out = []
    for bw, op in ((16, SCALAR_PHASE_16), (24, SCALAR_PHASE_24)):
        b = Batch(op)
        for name, k, s in phase_pairs():
            b.add(name, words(k, 8) + words(s, 8), 0, _phase_check(k, s, bw),
                  exact=band(euclid(k)[0]) != "mid")
        out.append(b)
    return out


_GROUPS = {"barrett": _g_barrett, "addneg": _g_addneg, "recode": _g_recode, "half": _g_half,
           "phase": _g_phase}
GROUPS = list(_GROUPS)
_cache = {}


def batches(which):
    """The batches by group name (computed once, shared by the CPU and GPU tests)."""
    if which not in _cache:
        _cache[which] = _GROUPS[which]()
    return _cache[which]
