"""Every device field primitive of lcpc_amd/csrc/field_dev.h and field_ln.h, called once per lane through tests/fe_harness.py on the
operand sets of tests/test_fe_cases.py and held to that module's Python-int models: exact equality for the packed layer and the exact
reductions; for the lazy limb layer equality mod p (or of the value, where the contract fixes it), the promised range, and normalised
limbs.  A whole set runs in ONE launch; it then runs reversed (the results must be the reversed results: the inline-assembly carry
chains keep per-lane state in VCC) and, where the set is a multiple of 64 long, once more without its last lane.  Output buffers are
sentinel-filled with one spare element that must stay untouched (fe_harness._done)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_harness as H  # noqa: E402
import test_fe_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _hex(x):
    if isinstance(x, int):
        return ("-0x%x" % -x) if x < 0 else "0x%x" % x
    return "[" + ", ".join(_hex(v) for v in x) + "]"


def run_set(what, cases, launch, judge):
    """launch(cases) -> one output per case (one device launch); judge(case, out) -> None, or what the model expected"""
    assert cases
    out = launch(cases)
    assert len(out) == len(cases)
    bad = [(c, o, m) for c, o in zip(cases, out) for m in [judge(c, o)] if m is not None]
    if bad:
        lines = ["%s: %d of %d lanes wrong; the first:" % (what, len(bad), len(cases))]
        lines += ["  operands %s\n    device %s\n    model  %s" % (_hex(c), _hex(o), m) for c, o, m in bad[:12]]
        pytest.fail("\n".join(lines))
    assert launch(cases[::-1]) == out[::-1], "%s: a lane's result depends on its position (reversed set)" % what
    if len(cases) % 64 == 0:
        assert launch(cases[:-1]) == out[:-1], "%s: a launch that ends inside a wave" % what
    return out


def exact(model):
    def judge(c, o):
        w = model(c)
        return None if o == w else _hex(w)
    return judge


# ---- packed layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["add", "sub", "mul"])
@pytest.mark.parametrize("fid", K.FIDS)
def test_binop(fid, op):
    F = K.fld(fid)
    code, model = {"add": (H.OP_ADD, K.m_add), "sub": (H.OP_SUB, K.m_sub), "mul": (H.OP_MUL, K.m_mul)}[op]
    run_set("fe_%s<%d>" % (op, F.NL), K.binary_pairs(fid, op),
            lambda cs: H.binop(code, fid, [a for a, _ in cs], [b for _, b in cs]), exact(lambda c: model(F, *c)))


@pytest.mark.parametrize("fid", K.FIDS)
def test_canon(fid):
    F = K.fld(fid)
    run_set("fe_canon<%d>" % F.NL, K.edge_set(fid), lambda cs: H.canon(fid, cs), exact(lambda a: K.m_canon(F, a)))


@pytest.mark.parametrize("form", ["t", "t_top"])
@pytest.mark.parametrize("fid", K.FIDS)
def test_reduce_once(fid, form):
    F = K.fld(fid)

    def launch(cs):
        if form == "t":
            assert all(T < F.R for T in cs)
            return H.reduce_once(fid, cs)
        return H.reduce_once(fid, [K.split_top(F, T)[0] for T in cs], [K.split_top(F, T)[1] for T in cs])

    run_set("fe_reduce_once<%d>(%s)" % (F.NL, form), K.reduce_once_set(fid), launch, exact(lambda T: K.m_reduce_once(F, T)))


@pytest.mark.parametrize("k", K.WIDE_KS)
@pytest.mark.parametrize("fid", K.FIDS)
def test_wide_dot(fid, k):
    F = K.fld(fid)
    run_set("wide_mac x %d + wide_reduce <%d>" % (k, F.NL), K.wide_dot_set(fid, k),
            lambda cs: H.wide_dot(fid, [a for a, _ in cs], [b for _, b in cs], k), exact(lambda c: K.m_wide(F, *c)[0]))


# ---- limb layer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", K.FIDS)
def test_from_packed_to_packed(fid):
    """from_packed is the model's split at every limb / word straddle, and to_packed undoes it for every a < 2^(32 NL), all ones included"""
    F = K.fld(fid)
    S = K.packed_any_set(fid)
    limbs = run_set("ln::from_packed", S, lambda cs: H.from_packed(fid, F.N, cs), exact(lambda a: K.m_from_packed(F, a)))
    assert all(K.pre_to_packed(F, l) for l in limbs)
    run_set("ln::to_packed", limbs, lambda cs: H.to_packed(fid, F.N, cs), exact(lambda l: F.value(l)))
    assert H.to_packed(fid, F.N, limbs) == S


def limb_judge(F, value=None, mod=None, lo=None, hi=None, hi_incl=False):
    """the result is normalised; its value is `value(case)` (exact) or congruent to `mod(case)`; it lies in [lo, hi) (or (lo, hi])"""
    def judge(c, o):
        v = F.value(o)
        ok = F.normalised(o)
        if value is not None:
            ok = ok and v == value(c)
        if mod is not None:
            ok = ok and (v - mod(c)) % F.p == 0
        if lo is not None:
            ok = ok and (lo < v <= hi if hi_incl else lo <= v < hi)
        if ok:
            return None
        want = "value %s" % _hex(value(c)) if value is not None else "== %s mod p" % _hex(mod(c) % F.p)
        return "%s, normalised, in %s%s, %s%s; got value %s = %.4f p" % (want, "(" if hi_incl else "[", _hex(lo) if lo is not None else "-",
                                                                       _hex(hi) if hi is not None else "-", "]" if hi_incl else ")", _hex(v), v / F.p)
    return judge


@pytest.mark.parametrize("fid", K.FIDS)
def test_normalize(fid):
    F = K.fld(fid)
    run_set("ln::normalize", K.normalize_set(fid), lambda cs: H.normalize(fid, F.N, cs), exact(lambda l: K.m_normalize(F, l)))


@pytest.mark.parametrize("fid", K.FIDS)
def test_clamp_q_clamp_apply(fid):
    """clamp_q's index is the model's floor division at every step of the estimate; clamp_apply with the negated table row returns
    V - q p, normalised, in [0, p + 64 B)"""
    F = K.fld(fid)
    nqp = K.clamp_table_negated(F)
    lo, hi = K.clamp_qa_range(F)

    def launch(cs):
        rows, q = H.clamp_qa(fid, F.N, cs, nqp)
        return [r + [i] for r, i in zip(rows, q)]

    def judge(c, o):
        want, i = K.m_clamp_qa(F, c)
        if o[-1] != i:
            return "index %d" % i
        return limb_judge(F, value=lambda _: F.value(want), lo=lo, hi=hi)(c, o[:-1])

    run_set("ln::clamp_q + clamp_apply", K.clamp_qa_set(fid), launch, judge)


@pytest.mark.parametrize("fid", K.FIDS)
def test_ln_mul(fid):
    """a w / R' mod p, normalised, in (-p - eps, eps]"""
    F = K.fld(fid)
    lo, hi = K.mul_range(F)
    run_set("ln::mul", K.mul_set(fid), lambda cs: H.mul(fid, F.N, [a for a, _ in cs], [w for _, w in cs]),
            limb_judge(F, mod=lambda c: K.m_mul_mod(F, *c), lo=lo, hi=hi, hi_incl=True))


@pytest.mark.parametrize("fid", K.LIMB_DOT_FIDS)
def test_mul_u(fid):
    """a w mod p for a wave-uniform w: one block of lanes per table, the operand set against each; normalised, inside wmul_bounds"""
    F = K.fld(fid)
    A, ws = K.mul_u_a_set(fid), K.mul_u_ws(fid)
    tabs = [K.shifted_multiples(F, w) for w in ws]
    lo, hi = K.mul_u_range(F)
    zero = [0] * F.N

    def launch(order):
        lanes = []
        for t in range(len(ws)):
            lanes += order + ([zero] * (256 - len(order)) if t + 1 < len(ws) else [])
        out = H.mul_u(fid, F.N, lanes, tabs)
        return [out[256 * t:256 * t + len(order)] for t in range(len(ws))]

    assert len(A) <= 256 and len(A) % 64
    out = launch(A)
    bad = []
    for w, rows in zip(ws, out):
        judge = limb_judge(F, mod=lambda a: F.value(a) * w, lo=lo, hi=hi)
        bad += [((a, w), o, m) for a, o in zip(A, rows) for m in [judge(a, o)] if m is not None]
    if bad:
        pytest.fail("\n".join(["ln::mul_u: %d lanes wrong; the first:" % len(bad)] +
                              ["  (a, w) %s\n    device %s\n    model  %s" % (_hex(c[0]) + ", " + _hex(c[1]), _hex(o), m) for c, o, m in bad[:12]]))
    assert launch(A[::-1]) == [rows[::-1] for rows in out], "ln::mul_u: a lane's result depends on its position"


@pytest.mark.parametrize("k", K.LAZY_KS)
@pytest.mark.parametrize("fid", K.LIMB_DOT_FIDS)
def test_lazy_dot(fid, k):
    """lazy_mac x k with a lazy_normalize at the cadence the kernels use, one lazy_reduce: the dot product / R' mod p, fully reduced"""
    import test_lazy_bounds as LB
    F = K.fld(fid)
    cad = {v[0][0] for v in LB.lazy29_cadences().values()}
    assert len(cad) == 1
    c = cad.pop()
    run_set("lazy_mac x %d / normalize every %d / lazy_reduce" % (k, c), K.lazy_dot_set(fid, k),
            lambda cs: H.lazy_dot(fid, F.N, [x for x, _ in cs], [v for _, v in cs], k, c), exact(lambda cv: K.m_lazy_dot(F, *cv)))


# ---- Ft255 only -----------------------------------------------------------------------------------------------------------------------
def test_clamp9():
    """ln::clamp: V - q p, normalised, in [0, p + 2^239)"""
    F = K.fld(3)
    qp = K.clamp_table(F)
    run_set("ln::clamp", K.clamp9_set(), lambda cs: H.clamp9(cs, qp),
            limb_judge(F, value=lambda l: F.value(K.m_clamp9(F, l)), lo=0, hi=F.p + (1 << 239)))


def test_to_packed_reduced():
    F = K.fld(3)
    qp = K.clamp_table(F)
    run_set("ln::to_packed_reduced", K.clamp9_set(), lambda cs: H.clamp9(cs, qp, reduced=True), exact(lambda l: F.value(l) % F.p))


def test_mul_r29():
    F = K.fld(3)
    run_set("fe_mul_r29", K.r29_set(), lambda cs: H.mul_r29([a for a, _ in cs], [b for _, b in cs]), exact(lambda c: K.m_lazy_dot(F, [c[0]], [c[1]])))


def test_canon_r29_is_canon():
    """fe_canon_r29 == fe_canon<8> == a / 2^256 mod p on the whole edge set, the random values included"""
    F = K.fld(3)
    E = K.edge_set(3)
    assert set(K.random_set(3)) <= set(E)
    got = run_set("fe_canon_r29", E, H.canon_r29, exact(lambda a: K.m_canon(F, a)))
    assert got == H.canon(3, E)


def test_harness_refuses_out_of_contract_calls():
    """a table index outside the 64 rows, a cadence or a term count past field_ln.h's limits: refused before anything is launched"""
    F = K.fld(3)
    far = [0] * 8 + [64 * F.PTOP1]
    with pytest.raises(H.BadArgs):
        H.clamp_qa(3, 9, [far], K.clamp_table_negated(F))
    with pytest.raises(H.BadArgs):
        H.clamp9([far], K.clamp_table(F))
    with pytest.raises(H.BadArgs):
        H.lazy_dot(3, 9, [[1] * 61], [[F.limbs(1)] * 61], 61, 6)
    with pytest.raises(H.BadArgs):
        H.lazy_dot(3, 9, [[1]], [[F.limbs(1)]], 1, 7)
    with pytest.raises(H.BadArgs):
        H.mul_u(0, 3, [[0, 0, 0]], [[0] * 9])
