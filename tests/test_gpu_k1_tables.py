"""The tables the Ligero row NTT (K1) reads, as the PRODUCT builds them (ctx.cpp: roots, wmul_table, clamp_table; kernels.hip roots_kernel;
ntt_lns.hip: roots_ln_kernel, lns_subtable_kernel and the five pack kernels), held to the contracts the multipliers state for them
(tests/k1_tables.py): ln::mul wants its twiddle normalised in [0, p), ln::mul2 both entries of its pair, ln::mul_u the balanced shifted
multiples, ln::clamp (i - 24) p as normalised signed limbs.  The range proofs and the direct primitive tests assume exactly these forms,
and a table with the right residues in another form still commits correctly on almost every input -- so the end-to-end comparisons with
the oracle cannot see it.  Exact Python integers throughout; no tolerances.

One context per case, made by lcpc_ctx_create and read through tests/native/k1_harness.cpp; no pass kernel runs.  S = log_n - 10 selects
the first-pass kernel's shape, so log_n = 11 .. 20 reach all ten.  Every case first asserts that the plan it asked for is the plan it
got.  Tables are compared in full up to 2^14 columns; above, the representation of every entry is checked vectorised and the exact value
at i in {0, 1, 2, n/4 - 1, n/4, n/2 - 1} and 4096 seeded indices.  Packs: every class of a pass with at most 16, else 16 of them
(k1_tables.sample_classes).  Every entry of a sampled class is checked for representation, membership AND its exact value: the index rule
of the DIF / K1n packs is restated in k1_tables (dif_*), that of the pure / coset form is tests/ntt_coset_rules.py's.

The K1n family as asked for is fid 0, 1, 2 x log_n 11 .. 20, but ctx.cpp plans Ft63 at 2^11, 2^12 and Ft127 at 2^11 as ONE pass of the
general kernel (a 2^12- / 2^11-element tile holds the row: common.FIRST_TWO_PASS): no K1n plan exists for them through lcpc_ctx_create.
Those three cases stay in the list, assert that one general pass explicitly and check d_roots, the only table such a context has;
first-pass shape S = 1 of Ft63 is reached by its three-pass case (2^21 columns).

Each case prints one line of counts (`k1-tables {...}`): entries checked in full and by sample."""
import json
import os
import re

import pytest

import common as CM
import k1_harness as K1
import k1_tables as T
from test_fe_cases import fld

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = list(range(11, 21))


def mul2_supported(s, first):
    """kernels.h ntt_l9s_mul2_supported, restated (test_the_restated_predicate_is_the_header_s holds it to the header's text)"""
    return s == 10 if not first else (1 <= s <= 10 and s not in (2, 7, 9))


def _fail(findings, what):
    assert not findings, "%s: %d finding(s)%s\n  %s" % (what, len(findings) + findings.dropped, " (first %d)" % len(findings) if findings.dropped else "",
                                                        "\n  ".join(findings))


def _tables(cx, F, case, counts):
    """every table the context has.  d_roots always; the limb tables, the clamp table and the fourth root's multiples where they exist"""
    log_n, n = cx.log_n, 1 << cx.log_n
    w = CM.ntt_root(cx.fid, log_n)
    half = max(n // 2, 1)
    assert cx.entries["d_roots"] == half
    idx = T.sample_indices(half, log_n, (case, "roots"))
    _fail(T.check_roots(F, w, cx.table("d_roots"), idx), "d_roots")
    counts["d_roots"] = (half, len(idx))
    if not cx.entries["d_rootsl"]:
        assert not any(cx.entries[t] for t in K1.TABLES[1:]), cx.entries
        return
    assert cx.entries["d_rootsl"] == cx.entries["d_rootslc"] == half and cx.entries["d_qpl"] == 64 and cx.entries["d_wq_w"] == 1, cx.entries
    full = {}
    for name, conv in (("d_rootsl", False), ("d_rootslc", True)):
        full[name] = cx.table(name)
        assert full[name].shape == (half, F.STRIDE)
        _fail(T.check_limb_table(F, w, full[name], idx, conv, name=name), name)
        counts[name] = (half, len(idx))
    _fail(T.check_clamp(F, cx.table("d_qpl")), "d_qpl")
    _fail(T.check_wq(F, cx.table("d_wq_w")), "d_wq_w")
    counts["d_qpl"], counts["d_wq_w"] = (64, 64), (1, 1)
    if len(cx.passes) == 3 and cx.passes[0].kind != "general":
        s0 = log_n - 20
        assert cx.entries["d_rootsls"] == cx.entries["d_rootslcs"] == 1 << 19
        for name, src in (("d_rootsls", "d_rootsl"), ("d_rootslcs", "d_rootslc")):
            sub = cx.table(name)
            _fail(T.check_subtable(sub, full[src], s0, name), name)
            _fail(T.check_limb_repr(F, sub, name=name), name)
            counts[name] = (1 << 19, 1 << 19)
    else:
        assert cx.entries["d_rootsls"] == cx.entries["d_rootslcs"] == 0


def _packs(cx, F, case, counts):
    for p in cx.passes:
        if p.kind == "general":
            assert p.n_classes == 0 and p.records == 0
            continue
        assert p.n_classes == T.classes_of(p), p
        slots, utabs = T.pass_slots(F, p)
        assert p.records == (2 if p.mul2 else 1) * sum(nv * period for _, nv, period in slots) and p.n_utabs == len(utabs), p
        w = CM.ntt_root(cx.fid, p.log_n)                         # (a sub-plan pass of a three-pass plan: the root of its 2^20-point transform)
        classes = T.sample_classes(p.n_classes, (case, p.index))
        recs = cx.pack_entries(p.index, classes)
        _fail(T.check_pack_entries(F, p, recs, classes, w), "pack of %r" % p)
        counts["pack%d" % p.index] = (p.n_classes, len(classes), len(recs))
        if utabs:
            assert T.has_mul_u(F)
            urecs = cx.uniform(p.index, classes)
            _fail(T.check_uniform(F, p, urecs, classes, w), "shifted multiples of %r" % p)
            counts["uniform%d" % p.index] = (p.n_classes, len(classes), len(urecs))
        else:
            with pytest.raises(K1.BadArgs):
                cx.uniform(p.index, classes)


def _case(family, fid, log_n, env, expect, three_pass=False):
    """expect: [(kernel kind, form, mul2)] per pass"""
    F, n = fld(fid), 1 << log_n
    case = "%s-ft%d-2^%d" % (family, CM.FIELD_BITS[fid], log_n)
    with K1.Ctx(fid, max(n // 2, 1), n, env=env) as cx:
        assert (cx.NL, cx.N, cx.W, cx.STRIDE, cx.log_n, cx.U_SLOT) == (F.NL, F.N, F.W, F.STRIDE, log_n, T.u_slot(F))
        got = [(p.kind, p.form, p.mul2) for p in cx.passes]
        if three_pass and cx.passes[0].kind == "general":
            pytest.fail("%s: the context fell back to the general kernel's plan -- the three-pass plan's tables did not fit the device "
                        "(ctx.cpp build_limb_plan); this case needs them" % case)
        assert got == expect, "%s: asked for %s, the context planned %s" % (case, expect, cx.passes)
        model = CM.ntt_plan(fid, log_n, general="LCPC_NTT_GENERAL" in (env or {}))
        # (a sub-plan pass of a three-pass plan counts its stages inside the 2^20-point transform; the general kernel has no first-pass form)
        assert [(p.kind, p.t0 if p.kind == "general" or len(cx.passes) < 3 or p.index == 0 else p.t0 + log_n - 20, p.s, p.first) for p in cx.passes] == \
            [(m["kernel"], m["t0"], m["s"], m["first"] and m["kernel"] != "general") for m in model], (cx.passes, model)
        counts = {}
        _tables(cx, F, case, counts)
        _packs(cx, F, case, counts)
        with pytest.raises(K1.BadArgs):                           # out-of-range requests are refused before the device is touched
            cx.table("d_roots", cx.entries["d_roots"], 1)
        with pytest.raises(K1.BadArgs):
            cx.pack_entries(len(cx.passes), [0])
    print("k1-tables " + json.dumps({"case": case, "counts": counts}))


@pytest.mark.parametrize("log_n", [1, 2, 5, 10])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_general_kernel_tables(fid, log_n):
    """one pass of the general kernel: d_roots; Ft255's limb kernel reads d_rootsl / d_rootslc / d_qpl / d_wq_w as well"""
    _case("general", fid, log_n, None, [("general", 0, 0)])


def test_general_kernel_tables_forced_ft255():
    _case("general-forced", 3, 13, {"LCPC_NTT_GENERAL": "1"}, [("general", 0, 0)] * len(CM.general_passes(3, 13, True)))


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("fid", [0, 1, 2])
def test_k1n_tables_and_packs(fid, log_n):
    """both passes' packs, the shifted multiples of Ft127 / Ft191, and every table.  Below common.FIRST_TWO_PASS the context plans one
    general pass (module docstring): asserted, and d_roots checked"""
    two = log_n >= CM.FIRST_TWO_PASS[fid]
    assert two or (fid, log_n) in ((0, 11), (0, 12), (1, 11))
    _case("K1n", fid, log_n, None, [("K1n", 0, 0)] * 2 if two else [("general", 0, 0)])


@pytest.mark.parametrize("log_n", LOGS)
def test_k1s_dif_tables_and_packs(log_n):
    _case("K1s-dif", 3, log_n, {"LCPC_NTT_FORM": "dif"}, [("K1s", 0, 0)] * 2)


@pytest.mark.parametrize("log_n", LOGS)
def test_k1s_coset_mont_packs_at_exact_indices(log_n):
    _case("K1s-coset-mont", 3, log_n, {"LCPC_NTT_FORM": "coset", "LCPC_NTT_MUL": "mont"}, [("K1s", 1, 0)] * 2)


@pytest.mark.parametrize("log_n", LOGS)
def test_k1s_coset_split_pairs(log_n):
    """the passes that report mul2 are exactly those of ntt_l9s_mul2_supported; their pairs are b0 = e 2^-116, b1 = e 2^29"""
    env = {"LCPC_NTT_MUL": "split"}
    if log_n < 16:
        env["LCPC_NTT_FORM"] = "coset"                            # (the default below 2^16 columns is the DIF form, which has no ln::mul2)
    _case("K1s-coset-split", 3, log_n, env, [("K1s", 1, int(mul2_supported(log_n - 10, True))), ("K1s", 1, int(mul2_supported(10, False)))])


@pytest.mark.parametrize("fid", [3, 0])
def test_three_pass_subtables_and_packs(fid):
    """2^21 columns: the 2^20-point subtables in full (every word of 2^19 entries, both tables), the first pass's pack (S = 1, 2048
    classes) and the two sub-plan passes' packs"""
    _case("3pass", fid, 21, None, [("K1s" if fid == 3 else "K1n", 0, 0)] * 3, three_pass=True)


@pytest.mark.parametrize("fid,log_n", [(0, 22), (1, 21)])
def test_k1n_first_pass_shapes_only_a_three_pass_plan_reaches(fid, log_n):
    """Ft63's first-pass shape S = 2 and Ft127's S = 1: the sizes at which a two-pass plan would have them are one-pass rows (module
    docstring), so their packs exist in three-pass plans only"""
    _case("3pass", fid, log_n, None, [("K1n", 0, 0)] * 3, three_pass=True)


def test_the_restated_predicate_is_the_header_s():
    src = open(os.path.join(ROOT, "lcpc_amd", "csrc", "kernels.h")).read()
    assert "constexpr bool ntt_l9s_mul2_supported(uint32_t s, bool first) { return !first ? s == 10 : (s >= 1 && s <= 10 && s != 2 && s != 7 && s != 9); }" in src
    assert [s for s in range(0, 12) if mul2_supported(s, True)] == [1, 3, 4, 5, 6, 8, 10] and [s for s in range(0, 12) if mul2_supported(s, False)] == [10]


PLAN_LINE = re.compile(r"ntt plan 2\^(\d+) pass (\d)/(\d): (K1s|K1n) s=(\d+) form=(\d) mul2=(\d)")


@pytest.mark.parametrize("fid,log_n,env", [(3, 18, {}), (3, 18, {"LCPC_NTT_MUL": "split-pure"}), (3, 13, {"LCPC_NTT_FORM": "coset", "LCPC_NTT_MUL": "split"}),
                                           (3, 17, {"LCPC_NTT_MUL": "split"}), (3, 14, {}), (1, 12, {}), (3, 21, {})])
def test_plan_report_is_the_plan_line_on_stderr(capfd, fid, log_n, env):
    """the harness's plan report against the line build_limb_plan writes under LCPC_DEBUG_TIMING (what tests/test_gpu_ntt_mul2.py parses)"""
    capfd.readouterr()
    with K1.Ctx(fid, 1 << (log_n - 1), 1 << log_n, env=dict(env, LCPC_DEBUG_TIMING="1")) as cx:
        passes = list(cx.passes)
    err = capfd.readouterr().err
    lines = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)), int(m.group(6)), int(m.group(7))) for m in PLAN_LINE.finditer(err)]
    assert lines and lines == [(log_n, p.index + 1, len(passes), p.kind, p.s, p.form, p.mul2) for p in passes], (err[-2000:], passes)
