"""One table cache behind both direct transform solvers (transform_solve.hpp):
a context that runs sine and cosine work in turn, sine first, must give what
fresh contexts give that ran one thing only.

The cache is keyed by (kind, n). (34, 34, 34) has n = 32 on all three axes:
one table per kind serves every axis, and both kinds meet at the same n, so a
cache keyed by n alone would hand the cosine passes the sine table.
(12, 9, 6) has three different n, all below one tile.

Every comparison is bitwise: the summation order of a pass is fixed, so the
tables alone decide the bits.
"""
import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from tests import dct_cases as KC
from tests import dst_cases as KS

pytestmark = pytest.mark.gpu

DST, DCT = A.HIP_POISSON_DST, A.HIP_POISSON_DCT
SHAPES = [(34, 34, 34), (12, 9, 6)]
# every transform of both kinds, interleaved: (kind, axis, inverse)
TRANSFORMS = [t for axis in range(3)
              for t in (("dst", axis, False), ("dct", axis, False), ("dct", axis, True))]


def _solve(ctx, shape, method):
    """(rc, status, iterations, (initial, final residual), x) of one solve."""
    if method == DST:
        rhs, x0 = KS.inputs(shape)
    else:
        rhs, _, x0 = KC.inputs(shape)
    x = np.array(x0)
    s, st = ctx.poisson_solve(method, x, rhs, *KS.spacing(shape))
    return s, st.status, st.iterations, (st.initial_residual, st.final_residual), x


def _transform(ctx, shape, which):
    kind, axis, inverse = which
    y = np.array(KS.inputs(shape)[1])
    if kind == "dst":
        s = ctx.dst_transform(y, axis)
    else:
        s = ctx.dct_transform(y, axis, inverse)
    return s, y


def _fresh(shape, fn, *args):
    ctx = api.HipProjection(*shape)
    try:
        return fn(ctx, shape, *args)
    finally:
        ctx.close()


def _same_solve(got, want, what):
    assert got[:4] == want[:4], (what, got[:4], want[:4])
    assert np.array_equal(got[4], want[4]), f"{what}: x differs from the fresh context's"


@pytest.mark.parametrize("shape", SHAPES, ids=KS.sid)
def test_one_cache_serves_both_kinds(hip_lib, shape):
    ref_solve = {m: _fresh(shape, _solve, m) for m in (DST, DCT)}
    for m, r in ref_solve.items():
        assert (r[0], r[1], r[2]) == (A.CFD_SUCCESS, A.POISSON_CONVERGED, 1), (m, r[:4])
    ref_tr = {t: _fresh(shape, _transform, t) for t in TRANSFORMS}
    for t, (s, _) in ref_tr.items():
        assert s == A.CFD_SUCCESS, (t, _native.last_error())
    ctx = api.HipProjection(*shape)
    try:
        for m in (DST, DCT):  # sine first: its tables are in the cache at every n
            _same_solve(_solve(ctx, shape, m), ref_solve[m], f"first pass, method {m}")
        for t in TRANSFORMS:
            s, y = _transform(ctx, shape, t)
            assert s == ref_tr[t][0], t
            assert np.array_equal(y, ref_tr[t][1]), f"{t}: differs from the fresh context's"
        for m in (DCT, DST):
            _same_solve(_solve(ctx, shape, m), ref_solve[m], f"second pass, method {m}")
    finally:
        ctx.close()
