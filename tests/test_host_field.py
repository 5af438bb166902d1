"""host_field.h's h_add / h_sub / h_mul / h_canon -- what verify, the Fiat-Shamir glue and the table builders compute with -- called
directly (tests/native/fe_harness.cpp feh_host_op, no device involved) on the operand sets of tests/test_fe_cases.py: the edge set
crossed with itself and the pairs built to sit on the final subtraction and on the borrow, against the Python-int models.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_harness as H  # noqa: E402
import test_fe_cases as K  # noqa: E402

pytestmark = pytest.mark.skipif(not H.available(), reason="lcpc_amd/lib/liblcpc_fe_harness.so is not built (make -C lcpc_amd/csrc)")


def _check(what, cases, got, want):
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, "%s: %d of %d wrong; the first: %s" % (
        what, len(bad), len(cases), ["%s -> %x, model %x" % ([hex(x) for x in c], g, w) for c, g, w in bad[:12]])


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
@pytest.mark.parametrize("fid", K.FIDS)
def test_host_binop(fid, op):
    F = K.fld(fid)
    code, model = {"add": (H.OP_ADD, K.m_add), "sub": (H.OP_SUB, K.m_sub), "mul": (H.OP_MUL, K.m_mul)}[op]
    pairs = K.binary_pairs(fid, op)
    got = H.host_op(code, fid, [a for a, _ in pairs], [b for _, b in pairs])
    _check("h_" + op, pairs, got, [model(F, a, b) for a, b in pairs])


@pytest.mark.parametrize("fid", K.FIDS)
def test_host_canon(fid):
    F = K.fld(fid)
    E = K.edge_set(fid)
    _check("h_canon", [(a,) for a in E], H.host_op(H.OP_CANON, fid, E), [K.m_canon(F, a) for a in E])


def test_host_op_refuses_unknown_fields_and_ops():
    with pytest.raises(H.BadArgs):
        H.lib()
        H._check("feh_host_op", H.lib().feh_host_op(H.OP_ADD, 4, None, None, None, 0))
    with pytest.raises(H.BadArgs):
        H._check("feh_host_op", H.lib().feh_host_op(7, 0, None, None, None, 0))
