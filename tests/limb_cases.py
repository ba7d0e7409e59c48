"""Raw-limb operands for the limb-level tests of the field and point arithmetic
(tests/test_field_limbs_cpu.py on the CPU build, tests/test_gpu_field_limbs.py on the gfx950
build): named classes of 10-limb vectors (radix 2^25.5, narwhal_amd/csrc/nw_field.hpp) at the
limb bounds tests/test_field_bounds.py models, each with the exact integer it denotes, and
curve points in extended / cached / affine-niels form with every coordinate stuffed to a bound.

The reference here is Python integers mod p and the affine twisted-Edwards addition law; the
bounds are imported from the model, never restated. A plain module, not a conftest.
"""
import random

import numpy as np

from test_field_bounds import (L, L_, LP_PAIRS, MUL_PAIRS, P4, P15, P15_, S_L, S_L_, S_T, S_T_,
                               SQ_INPUTS, T, T_LP)

P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
GROUP_L = 2**252 + 27742317777372353535851937790883648493
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]      # bit position of limb i
BITS = [26, 25] * 5
M = [(1 << b) - 1 for b in BITS]                          # M26 / M25

# operation codes: tools/limb_ops.hpp (hc_fe_ops / hc_ge_ops, k_fe_ops)
(FE_MUL, FE_SQ, FE_SQN, FE_ADD, FE_SUB, FE_SUB_NC, FE_NEG, FE_NEG_NC, FE_CARRY, FE_CANONICAL,
 FE_TOBYTES, FE_FROMBYTES, FE_ISZERO, FE_EQ, FE_ISNEGATIVE, FE_INVERT, FE_POW22523) = range(17)
(GE_DBL, GE_ADD_CACHED, GE_SUB_CACHED, GE_ADD_NIELS, GE_ADD_ANY, GE_ADD_ANY_NEGC) = range(32, 38)
# tools/lpcheck.hip (k_lp_ops)
(LP_MUL, LP_CARRY32, LP_SUB, LP_SUB_NC, LP_ROWS_OF, LP_SEL, LP_IDENTITY, LP_DBL, LP_ADD,
 LP_TO_CACHED, LP_CACHED_COMPONENT, LP_NIELS_COMPONENT, LP_IS_IDENTITY, LP_SQN, LP_POW22523,
 LP_CHAIN) = range(16)


def value(limbs):
    """The integer a limb vector denotes (not reduced)."""
    return sum(int(x) << OFF[i] for i, x in enumerate(limbs))


def tight(n):
    """Limbs of 0 <= n < 2^255, every limb below 2^26 / 2^25."""
    assert 0 <= n < 2**255
    return [(n >> OFF[i]) & M[i] for i in range(10)]


def fits(limbs, bound):
    return all(0 <= a <= b for a, b in zip(limbs, bound))


def stuff(v, bound, k=None, low=True):
    """A form of v mod p inside `bound` that sits AT the bound: v + k p (k the largest that
    fits unless given) with units moved between neighbouring limbs, either down (low: limb i
    full before limb i + 1 takes anything more than it must) or up (limb i + 1 full first)."""
    v %= P
    kmax = (value(bound) - v) // P
    assert kmax >= 0
    k = kmax if k is None else min(k, kmax)
    r = v + k * P
    out = [0] * 10
    for i in range(9, 0, -1):
        if low:
            need = r - value(bound[:i])
            li = 0 if need <= 0 else -(-need >> OFF[i])
        else:
            li = min(bound[i], r >> OFF[i])
        assert 0 <= li <= bound[i]
        out[i] = li
        r -= li << OFF[i]
    assert 0 <= r <= bound[0]
    out[0] = r
    assert value(out) % P == v
    return out


def carry_pass(h):
    """One sequential carry pass over limbs (limb 9's carry times 19 into limb 0, then limb 0's
    into limb 1): used only to BUILD the input form a carried difference leaves."""
    h = list(h)
    for i in range(9):
        h[i + 1] += h[i] >> BITS[i]
        h[i] &= M[i]
    h[0] += 19 * (h[9] >> 25)
    h[9] &= M[9]
    h[1] += h[0] >> 26
    h[0] &= M[0]
    return h


P_LIMBS = tight(P - 1)
P_LIMBS[0] += 1                                   # 2^26 - 19, M25, M26, ...: the limbs of p
ZEROS = {
    "p": P_LIMBS,
    "2p": [2 * x for x in P_LIMBS],
    "4p": list(P4),
    "sub(a,a)": carry_pass(P4),                   # a + 4p - a, carried
}
VALUES = [0, 1, 2, 19, P - 1, P - 19, P - 2**128, 2**255 - 20 - 2**25, 2**254 + 2**127 + 12345]


def unary(bound, seed, nrand=512, nstuff=24):
    """[(name, limbs)] for one operand whose limbs may reach `bound`."""
    rng = random.Random(seed)
    out = [("zero", [0] * 10), ("one", [1] + [0] * 9), ("p-1", tight(P - 1)),
           ("max", list(bound)), ("M26/M25", list(M))]
    out += [("zero as " + n, list(z)) for n, z in ZEROS.items() if fits(z, bound)]
    out += [(f"one-hot {i}", [bound[j] if j == i else 0 for j in range(10)]) for i in range(10)]
    # what fe_join can leave: limb 1 = 2^25 and limb 6 = 2^26 exactly
    for name, rest in (("0", [0] * 10), ("M", list(M))):
        for which in ((1,), (6,), (1, 6)):
            x = list(rest)
            for j in which:
                x[j] = 1 << BITS[j]
            if fits(x, bound):
                out.append((f"join limbs {which} = 2^bits, rest {name}", x))
    vals = VALUES + [rng.randrange(P) for _ in range(nstuff)]
    for n, v in enumerate(vals):
        out.append((f"stuffed low {v % 1000}", stuff(v, bound, low=True)))
        out.append((f"stuffed high {v % 1000}", stuff(v, bound, low=False)))
        if n % 3 == 0:
            kmax = (value(bound) - v) // P
            out.append((f"stuffed low k {v % 1000}", stuff(v, bound, k=rng.randint(0, kmax))))
    out += [(f"random {n}", [rng.randint(0, b) for b in bound]) for n in range(nrand)]
    for name, x in out:
        assert fits(x, bound), name
    return out


def binary(F, G, seed, nrand=512):
    """[(name, f, g)] for a (first, second) operand pair with bounds F, G: the named classes
    crossed, all 100 one-hot pairs (each product term alone in its column, with its x2 / x19
    / x38), stuffed against stuffed, and random against random."""
    uf, ug = unary(F, seed, nrand), unary(G, seed + 1, nrand)
    named_f = [c for c in uf if not c[0].startswith(("random", "one-hot", "stuffed"))]
    named_g = [c for c in ug if not c[0].startswith(("random", "one-hot", "stuffed"))]
    out = [(a + " * " + b, x, y) for a, x in named_f for b, y in named_g]
    out += [(f"one-hot {i} * one-hot {j}", [F[t] if t == i else 0 for t in range(10)],
             [G[t] if t == j else 0 for t in range(10)]) for i in range(10) for j in range(10)]
    sf = [c for c in uf if c[0].startswith("stuffed")]
    sg = [c for c in ug if c[0].startswith("stuffed")]
    out += [(a + " * " + b, x, y) for (a, x), (b, y) in zip(sf, sg)]
    out += [(a + " * " + b, x, y) for (a, x), (b, y) in zip(sf, reversed(sg))]
    out += [(a + " * max", x, list(G)) for a, x in sf[:8]] + [("max * " + b, list(F), y) for b, y in sg[:8]]
    rf = [c for c in uf if c[0].startswith("random")]
    rg = [c for c in ug if c[0].startswith("random")]
    out += [(a + " * " + b, x, y) for (a, x), (b, y) in zip(rf, rg)]
    return out


def distinct_pairs(pairs):
    seen, out = set(), []
    for name, (F, G) in pairs:
        key = (tuple(F), tuple(G))
        if key not in seen:
            seen.add(key)
            out.append((name, F, G))
    return out


FE_MUL_PAIRS = distinct_pairs(list(MUL_PAIRS.items()))
FE_SQ_INPUTS = list(SQ_INPUTS.items())
LP_MUL_PAIRS = distinct_pairs([(f"lp pair {i}", fg) for i, fg in enumerate(LP_PAIRS)])


# ---- the curve: -x^2 + y^2 = 1 + d x^2 y^2, affine, Python integers -----------------------
IDENTITY = (0, 1)


def inv(x):
    return pow(x, P - 2, P)


def on_curve(pt):
    x, y = pt
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def ed_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % P, (y1 * y2 + x1 * x2) * inv(1 - t) % P)


def ed_neg(p):
    return ((-p[0]) % P, p[1])


def ed_mul(k, p):
    r = IDENTITY
    while k:
        if k & 1:
            r = ed_add(r, p)
        p = ed_add(p, p)
        k >>= 1
    return r


def _decompress(y, sign):
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x2 = u * inv(v) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if (x * x - x2) % P:
        return None
    return ((P - x) if (x & 1) != sign else x, y)


BASE = _decompress(4 * inv(5) % P, 0)
_points = None


def points():
    """[(name, (x, y))]: the identity, the other seven 8-torsion points, small and large
    multiples of B and their negatives, and B plus a torsion point."""
    global _points
    if _points is None:
        y, t8 = 2, None
        while t8 is None:                      # a point of order exactly 8
            q = _decompress(y, 0)
            y += 1
            if q is None:
                continue
            t = ed_mul(GROUP_L, q)
            if ed_mul(4, t) != IDENTITY:
                t8 = t
        out = [("identity" if j == 0 else f"[{j}]T8", ed_mul(j, t8)) for j in range(8)]
        rng = random.Random(8)
        for k in (1, 2, 3, 8, GROUP_L - 1, GROUP_L - 2, rng.randrange(GROUP_L), rng.randrange(GROUP_L)):
            out.append((f"[{k % 10**6}]B", ed_mul(k, BASE)))
        out.append(("B + T8", ed_add(BASE, t8)))
        out.append(("[5]B + [4]T8", ed_add(ed_mul(5, BASE), ed_mul(4, t8))))
        assert all(on_curve(p) for _, p in out)
        _points = out
    return _points


def ext_form(pt, bound, rng, z=None):
    """(X, Y, Z, T) limbs of pt with a random Z, every coordinate stuffed to `bound`."""
    x, y = pt
    z = rng.randrange(1, P) if z is None else z
    low = rng.random() < 0.5
    return [stuff(c, bound, low=low) for c in (x * z, y * z, z, x * y * z)]


def cached_form(pt, bound, bound_t2d, rng, z=None, neg_t2d=False):
    """(YpX, YmX, Z2, T2d) limbs; T2d (the first operand of its product, possibly an uncarried
    negation) stuffed to bound_t2d and negated in value when neg_t2d (ge_add_any_negc)."""
    x, y = pt
    z = rng.randrange(1, P) if z is None else z
    low = rng.random() < 0.5
    t2d = D2 * x * y * z
    return [stuff((y + x) * z, bound, low=low), stuff((y - x) * z, bound, low=low),
            stuff(2 * z, bound, low=low), stuff(-t2d if neg_t2d else t2d, bound_t2d, low=low)]


def niels_form(pt, bound, bound_t2d, rng, neg_t2d=False):
    """(ypx, ymx, xy2d) limbs of the affine point."""
    c = cached_form(pt, bound, bound_t2d, rng, z=1, neg_t2d=neg_t2d)
    return [c[0], c[1], c[3]]


def projective_equal(X, Y, Z, T, pt):
    """X/Z, Y/Z are pt and T Z = X Y, for limb vectors or integers."""
    X, Y, Z = [c if isinstance(c, int) else value(c) for c in (X, Y, Z)]
    if Z % P == 0:
        return False
    ok = (X - pt[0] * Z) % P == 0 and (Y - pt[1] * Z) % P == 0
    if T is not None:
        T = T if isinstance(T, int) else value(T)
        ok = ok and (T * Z - X * Y) % P == 0
    return ok


# ---- packing ------------------------------------------------------------------------------
def lp_plane(rows, garbage=None):
    """64 words of a limb-parallel operand: row r's limbs in lanes 16 r .. 16 r + 9; lanes
    10..15 hold 0, or values from `garbage` (a random.Random)."""
    out = []
    for r in rows:
        out += list(r) + [garbage.getrandbits(32) if garbage else 0 for _ in range(6)]
    return out


def lp_rows(plane):
    """The four 10-limb rows and the 24 dead-lane words of a 64-word plane."""
    plane = [int(x) for x in plane]
    return [plane[16 * r:16 * r + 10] for r in range(4)], [plane[16 * r + k] for r in range(4) for k in range(10, 16)]


# the model's bound shapes by name (per-lane code; the same shapes over T_LP end in "_")
BOUNDS = {"T": T, "L": L, "P15": P15, "S_T": S_T, "S_L": S_L, "P4": P4, "T_LP": T_LP, "L_": L_,
          "P15_": P15_, "S_T_": S_T_, "S_L_": S_L_}


# ---- batches: cases of one operation with their checks --------------------------------------
class Batch:
    """Cases of one operation code. cases: (name, A, B, k, check) with A / B the operand's
    words (a limb vector, or a list of them laid end to end) and check(out words) asserting."""

    def __init__(self, op, words):
        self.op, self.words, self.cases = op, words, []

    def add(self, name, A, B, k, check):
        self.cases.append((name, A, B, k, check))

    def arrays(self):
        def flat(v):
            return [x for part in v for x in part] if v and isinstance(v[0], (list, tuple)) else list(v)
        n = len(self.cases)
        A = np.zeros((n, self.words), np.uint32)
        B = np.zeros((n, self.words), np.uint32)
        for i, (_, a, b, _, _) in enumerate(self.cases):
            a, b = flat(a), flat(b)
            A[i, :len(a)] = a
            B[i, :len(b)] = b
        return A, B, np.array([c[3] for c in self.cases], np.int32)

    def check(self, out):
        assert len(out) == len(self.cases)
        for (name, _, _, _, chk), row in zip(self.cases, out.tolist()):
            try:
                chk(row)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None


def _is(expected, bound):
    """The first 10 words denote `expected` mod p and every limb is within `bound`."""
    def chk(o):
        r = o[:10]
        assert value(r) % P == expected % P, ("value", r)
        assert fits(r, bound), ("limb over its bound", r, bound)
    return chk


def _exact(words):
    def chk(o):
        assert o[:len(words)] == list(words), ("got", o[:len(words)], "want", list(words))
    return chk


def _vadd(a, b):
    return [x + y for x, y in zip(a, b)]


_cache = {}


def fe_batches(which):
    """The per-lane batches by group name (computed once, shared by the CPU and GPU tests)."""
    if which not in _cache:
        _cache[which] = _FE_GROUPS[which]()
    return _cache[which]


def _g_mul():
    b = Batch(FE_MUL, 40)
    for n, (name, F, G) in enumerate(FE_MUL_PAIRS):
        for cn, f, g in binary(F, G, 100 + 2 * n):
            b.add(f"fe_mul [{name}] {cn}", f, g, 0, _is(value(f) * value(g), T))
    return [b]


def _g_sq():
    b, bn = Batch(FE_SQ, 40), Batch(FE_SQN, 40)
    for n, (name, F) in enumerate(FE_SQ_INPUTS):
        u = unary(F, 200 + n)
        for cn, f in u:
            b.add(f"fe_sq [{name}] {cn}", f, [], 0, _is(value(f) ** 2, T))
        for j, (cn, f) in enumerate(u[:160]):
            k = (1, 2, 5, 10, 50)[j % 5]
            bn.add(f"fe_sqn {k} [{name}] {cn}", f, [], k, _is(pow(value(f), 2 ** k, P), T))
    return [b, bn]


def _g_addsub():
    out = []
    add = Batch(FE_ADD, 40)
    for n, (F, G, R) in enumerate(((T, T, L), (T, L, P15), (L, T, P15))):
        for cn, f, g in binary(F, G, 300 + 2 * n):
            add.add(f"fe_add {cn}", f, g, 0, _is(value(f) + value(g), R))
    out.append(add)
    # fe_sub / fe_sub_nc: the subtrahend's limbs may reach those of 4p (the header's domain)
    sub, snc = Batch(FE_SUB, 40), Batch(FE_SUB_NC, 40)
    n = 0
    for fn in ("T", "L", "P15"):
        for gn in ("T", "L", "P4"):
            F, G = BOUNDS[fn], BOUNDS[gn]
            n += 1
            for cn, f, g in binary(F, G, 320 + 2 * n):
                sub.add(f"fe_sub [{fn} - {gn}] {cn}", f, g, 0, _is(value(f) - value(g), T))
                snc.add(f"fe_sub_nc [{fn} - {gn}] {cn}", f, g, 0,
                        _is(value(f) - value(g), _vadd(F, P4)))
    # the two shapes the model names: S_T = fe_sub_nc(T, T), S_L = fe_sub_nc(L, T)
    for (F, S) in ((T, S_T), (L, S_L)):
        for cn, f, g in binary(F, T, 350):
            snc.add(f"fe_sub_nc -> S {cn}", f, g, 0, _is(value(f) - value(g), S))
    out += [sub, snc]
    neg, nnc = Batch(FE_NEG, 40), Batch(FE_NEG_NC, 40)
    for fn in ("T", "L", "P4"):
        for cn, f in unary(BOUNDS[fn], 360):
            neg.add(f"fe_neg [{fn}] {cn}", f, [], 0, _is(-value(f), T))
            nnc.add(f"fe_neg_nc [{fn}] {cn}", f, [], 0, _is(-value(f), P4))
    return out + [neg, nnc]


_REDUCE_INPUTS = ("T", "L", "P15", "S_T", "S_L")


def _g_reduce():
    car, can, tob = Batch(FE_CARRY, 40), Batch(FE_CANONICAL, 40), Batch(FE_TOBYTES, 40)
    zer, isn = Batch(FE_ISZERO, 40), Batch(FE_ISNEGATIVE, 40)
    for n, fn in enumerate(_REDUCE_INPUTS):
        for cn, f in unary(BOUNDS[fn], 400 + n):
            v = value(f) % P
            name = f"[{fn}] {cn}"
            car.add("fe_carry " + name, f, [], 0, _is(v, T))
            can.add("fe_canonical " + name, f, [], 0, _exact(tight(v)))
            tob.add("fe_tobytes " + name, f, [], 0,
                    _exact([(v >> (32 * j)) & 0xffffffff for j in range(8)]))
            zer.add("fe_iszero " + name, f, [], 0, _exact([1 if v == 0 else 0]))
            isn.add("fe_isnegative " + name, f, [], 0, _exact([v & 1]))
    assert sum(1 for c in zer.cases if value(c[1]) % P == 0) >= 30     # forms of zero
    return [car, can, tob, zer, isn]


def _g_eq():
    b = Batch(FE_EQ, 40)
    rng = random.Random(500)
    vals = VALUES + [rng.randrange(P) for _ in range(40)]
    for an in ("T", "L"):
        for bn in ("T", "L", "P4"):
            FA, FB = BOUNDS[an], BOUNDS[bn]
            for v in vals:
                forms_a = [stuff(v, FA, low=True), stuff(v, FA, low=False), stuff(v, FA, k=0)]
                for d in (0, 0, 1, P - 1, 2 * v, 19, 2 ** 255 - 19 - 2 ** 25):
                    w = (v + d) % P if d != 2 * v else (-v) % P
                    fb = stuff(w, FB, low=rng.random() < 0.5,
                               k=rng.choice((None, 0, 1)))
                    fa = rng.choice(forms_a)
                    b.add(f"fe_eq [{an}, {bn}] {v % 1000} {d % 1000}", fa, fb, 0,
                          _exact([1 if (v - w) % P == 0 else 0]))
            for zn, z in ZEROS.items():        # every zero against every zero
                for zn2, z2 in ZEROS.items():
                    if fits(z, FA) and fits(z2, FB):
                        b.add(f"fe_eq zero {zn} {zn2}", z, z2, 0, _exact([1]))
                        b.add(f"fe_eq zero {zn} one", z, [1] + [0] * 9, 0, _exact([0]))
    return [b]


def _g_bytes():
    b = Batch(FE_FROMBYTES, 40)
    rng = random.Random(600)
    ints = [0, 1, P - 1, P, P + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1, 2 ** 255 + P]
    ints += [1 << i for i in range(0, 256, 5)] + [rng.getrandbits(256) for _ in range(256)]
    for x in ints:
        words = [(x >> (32 * j)) & 0xffffffff for j in range(8)]
        b.add(f"fe_frombytes {x:#x}", words, [], 0, _exact(tight(x & (2 ** 255 - 1))))
    return [b]


def _g_pow():
    inv_, pw = Batch(FE_INVERT, 40), Batch(FE_POW22523, 40)
    for cn, f in unary(T, 700):
        v = value(f)
        inv_.add("fe_invert " + cn, f, [], 0, _is(pow(v, P - 2, P), T))
        pw.add("fe_pow22523 " + cn, f, [], 0, _is(pow(v, (P - 5) // 8, P), T))
    return [inv_, pw]


def _ge_check(expected, want_t):
    def chk(o):
        X, Y, Z, T_ = o[0:10], o[10:20], o[20:30], o[30:40]
        assert projective_equal(X, Y, Z, T_ if want_t else None, expected), ("point", o)
        for c in (X, Y, Z) + ((T_,) if want_t else ()):
            assert fits(c, T), ("limb over T", c)
    return chk


def _g_ge():
    rng = random.Random(800)
    pts = points()
    dbl = Batch(GE_DBL, 40)
    for name, pt in pts:
        for rep in range(4):
            want_t = rep != 3
            dbl.add(f"ge_dbl {name} #{rep}", ext_form(pt, T, rng), [], int(want_t),
                    _ge_check(ed_add(pt, pt), want_t))
    dbl.add("ge_dbl identity Z = 1", [[0] * 10, [1] + [0] * 9, [1] + [0] * 9, [0] * 10], [], 1,
            _ge_check(IDENTITY, True))
    bs = {op: Batch(op, 40) for op in (GE_ADD_CACHED, GE_SUB_CACHED, GE_ADD_NIELS, GE_ADD_ANY,
                                       GE_ADD_ANY_NEGC)}
    junk = [0xffffffff] * 10          # Z2 of an affine entry: never read
    for pn, p in pts:
        for qn, q in pts:
            name = f"{pn} + {qn}"
            s, d = ed_add(p, q), ed_add(p, ed_neg(q))
            want_t = rng.random() < 0.8
            k = int(want_t)
            P1 = ext_form(p, T, rng)
            # 2dT is the FIRST operand of its product and may be an uncarried negation: S_T
            Qc = cached_form(q, T, S_T, rng)
            bs[GE_ADD_CACHED].add("ge_add_cached " + name, P1, Qc, k, _ge_check(s, want_t))
            bs[GE_SUB_CACHED].add("ge_sub_cached " + name, P1, Qc, k, _ge_check(d, want_t))
            bs[GE_ADD_ANY].add("ge_add_any " + name, P1, Qc, k, _ge_check(s, want_t))
            Qn = niels_form(q, T, S_T, rng)
            bs[GE_ADD_NIELS].add("ge_add_niels " + name, P1, Qn, k, _ge_check(s, want_t))
            bs[GE_ADD_ANY].add("ge_add_any affine " + name, P1, [Qn[0], Qn[1], junk, Qn[2]],
                               k | 2, _ge_check(s, want_t))
            Qm = cached_form(q, T, S_T, rng, neg_t2d=True)
            bs[GE_ADD_ANY_NEGC].add("ge_add_any_negc " + name, P1, Qm, k, _ge_check(s, want_t))
            Qa = niels_form(q, T, S_T, rng, neg_t2d=True)
            bs[GE_ADD_ANY_NEGC].add("ge_add_any_negc affine " + name, P1,
                                    [Qa[0], Qa[1], junk, Qa[2]], k | 2, _ge_check(s, want_t))
    return [dbl] + list(bs.values())


_FE_GROUPS = {"mul": _g_mul, "sq": _g_sq, "addsub": _g_addsub, "reduce": _g_reduce, "eq": _g_eq,
              "bytes": _g_bytes, "pow": _g_pow, "ge": _g_ge}


# ---- limb-parallel batches (nw_lp.hpp through tools/lpcheck.hip k_lp_ops) --------------------
# One wave per case: four input planes of 64 words and four output planes. A case's check gets
# the 256 output words. IGNORES_DEAD: the operations whose results may not depend on what the
# inputs' lanes 10..15 hold; the others (lane-wise moves and the uncarried difference) pass
# those lanes through, so they hold 0 on output when they held 0 on input (nw_lp.hpp).
IGNORES_DEAD = {LP_MUL, LP_CARRY32, LP_SUB, LP_DBL, LP_ADD, LP_TO_CACHED, LP_IS_IDENTITY, LP_SQN,
                LP_POW22523, LP_CHAIN}


class LpBatch:
    def __init__(self, op):
        self.op, self.cases = op, []

    def add(self, name, planes, k, check):
        """planes: up to four operands, each four 10-limb rows (or 64 raw words)."""
        self.cases.append((name, planes, k, check))

    def arrays(self, garbage=False):
        """n x 256 input words and n integers; lanes 10..15 of every operand given as rows hold
        0, or random words when garbage."""
        rng = random.Random(99) if garbage else None
        A = np.zeros((len(self.cases), 256), np.uint32)
        for i, (_, planes, _, _) in enumerate(self.cases):
            for p, rows in enumerate(planes):
                w = rows if len(rows) == 64 else lp_plane(rows, rng)
                A[i, 64 * p:64 * p + 64] = w
        return A, np.array([c[2] for c in self.cases], np.int32)

    def check(self, out):
        assert len(out) == len(self.cases)
        for (name, _, _, chk), row in zip(self.cases, out.tolist()):
            try:
                chk(row)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None


def _lp_rows_are(expected, bound=None, exact=False, plane=0):
    """Row r of the output plane denotes expected[r] mod p (or equals it limb for limb), every
    live limb within `bound`, lanes 10..15 zero."""
    def chk(o):
        rows, dead = lp_rows(o[64 * plane:64 * plane + 64])
        assert not any(dead), ("lanes 10..15 not zero", dead)
        for r, (got, want) in enumerate(zip(rows, expected)):
            if want is None:
                continue
            if exact:
                assert got == list(want), ("row", r, got, want)
            else:
                assert value(got) % P == want % P, ("row value", r, got)
            if bound is not None:
                assert fits(got, bound[r] if isinstance(bound[0], list) else bound), ("row over bound", r, got)
    return chk


def _lp_point_is(expected, plane=0):
    def chk(o):
        rows, dead = lp_rows(o[64 * plane:64 * plane + 64])
        assert not any(dead), ("lanes 10..15 not zero", dead)
        assert projective_equal(rows[0], rows[1], rows[2], rows[3], expected), ("point", rows)
        for r in rows:
            assert fits(r, T_LP), ("limb over T_LP", r)
    return chk


def _both(*checks):
    def chk(o):
        for c in checks:
            c(o)
    return chk


def _by4(items):
    items = list(items)
    while len(items) % 4:
        items.append(items[-1])
    return [items[i:i + 4] for i in range(0, len(items), 4)]


def lp_tab(cached):
    """lp_add's row order (YmX, YpX, T2d, Z2) of a (YpX, YmX, Z2, T2d) cached form."""
    return [cached[1], cached[0], cached[3], cached[2]]


def lp_batches(which):
    key = "lp_" + which
    if key not in _cache:
        _cache[key] = _LP_GROUPS[which]()
    return _cache[key]


def _l_mul():
    b = LpBatch(LP_MUL)
    for n, (name, F, G) in enumerate(LP_MUL_PAIRS):
        for quad in _by4(binary(F, G, 1000 + 2 * n)):
            b.add(f"lp_mul [{name}] {quad[0][0]} ..", [[q[1] for q in quad], [q[2] for q in quad]], 0,
                  _lp_rows_are([value(q[1]) * value(q[2]) for q in quad], T_LP))
    return [b]


def _l_carry_sub():
    car, sub, snc = LpBatch(LP_CARRY32), LpBatch(LP_SUB), LpBatch(LP_SUB_NC)
    top = _vadd(P15_, P4)                       # the model: every difference stays below 2^29
    assert max(top) < 2 ** 29
    for n, bound in enumerate((T_LP, L_, P15_, S_T_, S_L_, top)):
        for quad in _by4(unary(bound, 1100 + n)):
            car.add(f"lp_carry32 {quad[0][0]} ..", [[q[1] for q in quad]], 0,
                    _lp_rows_are([value(q[1]) for q in quad], T_LP))
    n = 0
    for F in (T_LP, L_, P15_):
        for G in (T_LP, L_):
            n += 1
            for quad in _by4(binary(F, G, 1120 + 2 * n)):
                ops = [[q[1] for q in quad], [q[2] for q in quad]]
                want = [value(q[1]) - value(q[2]) for q in quad]
                sub.add(f"lp_sub {quad[0][0]} ..", ops, 0, _lp_rows_are(want, T_LP))
                snc.add(f"lp_sub_nc {quad[0][0]} ..", ops, 0, _lp_rows_are(want, _vadd(F, P4)))
    return [car, sub, snc]


def _l_moves():
    rng = random.Random(1200)
    rows_of, sel, ident = LpBatch(LP_ROWS_OF), LpBatch(LP_SEL), LpBatch(LP_IDENTITY)
    for i in range(32):
        x = [[rng.getrandbits(32) for _ in range(10)] for _ in range(4)]

        def chk(o, x=x):
            for p in range(4):       # r_p: row p of the input in every row
                _lp_rows_are([x[p]] * 4, exact=True, plane=p)(o)
        rows_of.add(f"lp_rows_of {i}", [x], 0, chk)
        ops = [[[rng.getrandbits(32) for _ in range(10)] for _ in range(4)] for _ in range(4)]
        sel.add(f"lp_sel {i}", ops, 0, _lp_rows_are([ops[r][r] for r in range(4)], exact=True))
    one = [1] + [0] * 9
    ident.add("lp_identity", [], 0, _lp_rows_are([[0] * 10, one, one, [0] * 10], exact=True))
    return [rows_of, sel, ident]


def _l_points():
    rng = random.Random(1300)
    pts = points()
    dbl, add, toc = LpBatch(LP_DBL), LpBatch(LP_ADD), LpBatch(LP_TO_CACHED)
    d2 = [tight(D2)] * 4
    one = [1] + [0] * 9
    for name, pt in pts:
        for rep in range(3):
            v = ext_form(pt, T_LP, rng)
            dbl.add(f"lp_dbl {name} #{rep}", [v], 0, _lp_point_is(ed_add(pt, pt)))
            X, Y, Z, T_ = [value(c) for c in v]
            toc.add(f"lp_to_cached {name} #{rep}", [v, d2], 0,
                    _lp_rows_are([Y - X, Y + X, T_ * D2, 2 * Z], T_LP))
    dbl.add("lp_dbl identity Z = 1", [[[0] * 10, one, one, [0] * 10]], 0, _lp_point_is(IDENTITY))
    for pn, p in pts:
        for qn, q in pts:
            s = ed_add(p, q)
            v = ext_form(p, T_LP, rng)
            # 2dT: the first operand of its product, possibly an uncarried negation
            add.add(f"lp_add {pn} + {qn}", [v, lp_tab(cached_form(q, T_LP, S_T_, rng))], 0,
                    _lp_point_is(s))
            n = niels_form(q, T_LP, S_T_, rng)
            add.add(f"lp_add {pn} + niels {qn}", [v, [n[1], n[0], n[2], [2] + [0] * 9]], 0,
                    _lp_point_is(s))
    return [dbl, add, toc]


def _l_components():
    rng = random.Random(1400)
    cc, nc = LpBatch(LP_CACHED_COMPONENT), LpBatch(LP_NIELS_COMPONENT)
    two = [2] + [0] * 9
    for i in range(16):
        c = [[rng.getrandbits(32) for _ in range(10)] for _ in range(4)]     # YpX YmX Z2 T2d
        mem = [x for part in c for x in part] + [rng.getrandbits(32) for _ in range(24)]
        cc.add(f"lp_cached_component {i}", [[0] * 64, mem], 0,
               _lp_rows_are(lp_tab(c), exact=True))
    for name, pt in points():
        n = niels_form(pt, T, T, rng)              # ypx, ymx, xy2d: a table entry, carried
        mem = n[0] + n[1] + n[2] + [rng.getrandbits(32) for _ in range(34)]
        x, y = pt
        nc.add(f"lp_niels_component +{name}", [[0] * 64, mem], 0,
               _lp_rows_are([n[1], n[0], n[2], two], exact=True))
        # neg: the niels form of -P = (-x, y): ymx' = y + x, ypx' = y - x, xy2d' = -2dxy
        nc.add(f"lp_niels_component -{name}", [[0] * 64, mem], 1, _both(
            _lp_rows_are([n[0], n[1], None, two], exact=True),
            _lp_rows_are([y + x, y - x, -D2 * x * y, 2], [T, T, P4, T])))
    return [cc, nc]


def _l_identity():
    rng = random.Random(1500)
    b = LpBatch(LP_IS_IDENTITY)
    zeros = [[0] * 10] + [z for z in ZEROS.values() if fits(z, S_T_)] + [stuff(0, T_LP), stuff(0, T_LP, low=False)]
    small = [1, 2, 12345, 2 ** 243 + 7]          # v + p still fits T_LP
    vals = small + [P - 1, rng.randrange(P), rng.randrange(P)]

    def case(name, X, Y, Z, want):
        junk = [rng.randint(0, t) for t in T_LP]
        b.add("lp_is_identity " + name, [[X, Y, Z, junk]], 0,
              lambda o: _exact([want] * 64)(o[:64]))
    for i, X in enumerate(zeros):
        for v in vals:
            Y, Z = tight(v), stuff(v, T_LP, low=bool(i & 1))
            if v in small:
                assert value(Z) - value(Y) == P          # they differ by a multiple of p
            case(f"zero form {i}, Y = Z = {v % 1000}", X, Y, Z, 1)
            case(f"zero form {i}, Y = Z + 1", X, stuff(v + 1, T_LP), Z, 0)
            case(f"zero form {i}, Y = -Z", X, stuff(-v, T_LP), Z, 0)       # (0, -1): order 2
    for v in vals:
        Y, Z = stuff(v, T_LP, k=0), stuff(v, T_LP)
        for X in ([1] + [0] * 9, stuff(1, T_LP), stuff(P - 1, T_LP, low=False), [0] * 9 + [1]):
            case(f"X != 0, Y = Z = {v % 1000}", X, Y, Z, 0)
    for name, pt in points():
        X, Y, Z, _ = ext_form(pt, T_LP, rng)
        case("point " + name, X, Y, Z, 1 if pt == IDENTITY else 0)
    return [b]


def _l_pow():
    rng = random.Random(1600)
    sqn, pw = LpBatch(LP_SQN), LpBatch(LP_POW22523)
    u = unary(T_LP, 1601)
    for j, quad in enumerate(_by4(u)):
        k = (1, 2, 5, 50)[j % 4]
        sqn.add(f"lp_sqn {k} {quad[0][0]} ..", [[q[1] for q in quad]], k,
                _lp_rows_are([pow(value(q[1]), 2 ** k, P) for q in quad], T_LP))
    zs = [0, 1, P - 1, 2, P - 2, 2 ** 255 - 20, 2 ** 254] + [rng.randrange(P) for _ in range(57)]
    forms = [tight(z) for z in zs]                                   # canonical z
    forms += [f for cn, f in u if not cn.startswith("random")]       # and product outputs (T_LP)
    for quad in _by4(forms):
        pw.add(f"lp_pow22523 {value(quad[0]) % 1000} ..", [quad], 0,
               _lp_rows_are([pow(value(f), (P - 5) // 8, P) for f in quad], T_LP))
    return [sqn, pw]


CHAIN_KS = (1, 8, 248)


def _l_chain():
    rng = random.Random(1700)
    b = LpBatch(LP_CHAIN)
    pts = points()
    for k in CHAIN_KS:
        for i, (pn, p) in enumerate(pts):
            qn, q = pts[(5 * i + k) % len(pts)]
            want = ed_add(ed_mul(2 ** k, p), q)

            def seen(o):      # plane 1: the per-lane maximum over the whole chain
                rows, dead = lp_rows(o[64:128])
                assert not any(dead), ("lanes 10..15 not zero in the chain", dead)
                for r in rows:
                    assert fits(r, T_LP), ("a limb of the chain over T_LP", r)
            b.add(f"chain [2^{k}] {pn} + {qn}",
                  [ext_form(p, T_LP, rng), lp_tab(cached_form(q, T_LP, S_T_, rng))], k,
                  _both(_lp_point_is(want), seen))
    return [b]


_LP_GROUPS = {"mul": _l_mul, "carry_sub": _l_carry_sub, "moves": _l_moves, "points": _l_points,
              "components": _l_components, "identity": _l_identity, "pow": _l_pow,
              "chain": _l_chain}
