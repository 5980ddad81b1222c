"""The MFMA reduction kernels that were judged by one number per tensor -- the stride-1 weight gradient (four kernels, three tile configurations behind
csrc/wgrad_plan.hpp), the strided weight gradient and csrc/pointwise.hip -- on integer operands, where bf16 and f32 accumulation are exact in any order
and the result must EQUAL the float64 reference at every element (tests/exact_ref.py; tests/test_exact_ref_cpu.py checks the instrument and that every
case below is exact).  A failure names the first differing element.  The rounding, which integers cannot see, is held separately on N(0, 1) operands at
derived per-element bounds (gpu_checks.check_pointwise_exact / check_wgrad_exact).  Run with -s to see the plan each stride-1 case ran and the worst
ratio of each real-valued case."""
import pytest
import torch

import exact_ref as er
import gpu_checks as gc
from test_gpu_mf_kernels import POINTWISE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X; the product path has no CPU fallback')
    from rsuper_amd.hip import lib
    lib.require_device()


def _ok(r):
    print(f"{r['name']}: err {r['err']:.3f} tol {r['tol']:.1f} ({r['note']})")
    assert r['ok'], f"{r['name']}: err {r['err']:.3e} > tol {r['tol']:.1e} ({r['note']})"


def _wid(c):
    return f"{c[0]}{c[1]}mt{c[2]}_{c[3]}_N{c[4]}_{'x'.join(map(str, c[5]))}_{c[6]}+{c[7]}to{c[8]}+{c[9]}_{c[10]}_thr{c[11]}_tr{c[12]}"


@pytest.mark.parametrize('case', er.WGRAD_INT, ids=_wid)
def test_wgrad_equals_float64_on_integer_operands(case):
    _ok(gc.check_wgrad_int(*case))


@pytest.mark.parametrize('mode,N,S,Ca,Ya,Yb', er.WGRAD_S2_INT)
def test_strided_wgrad_equals_float64_on_integer_operands(mode, N, S, Ca, Ya, Yb):
    _ok(gc.check_wgrad_s2_int(mode, N, S, Ca, Ya, Yb))


@pytest.mark.parametrize('mode,R,K,N', POINTWISE)
def test_pointwise_equals_float64_on_integer_operands(mode, R, K, N):
    _ok(gc.check_pointwise_int(mode, R, K, N))


@pytest.mark.parametrize('mode,R,K,N', er.POINTWISE_SLICED)
def test_pointwise_on_column_slices_equals_float64_on_integer_operands(mode, R, K, N):
    _ok(gc.check_pointwise_int(mode, R, K, N, True))


@pytest.mark.parametrize('R,K,N', [c[1:] for c in POINTWISE if c[0] == 'bf16' and c[1] <= 4160])
def test_pointwise_rounding_within_the_derived_bound(R, K, N):
    _ok(gc.check_pointwise_exact(R, K, N))


@pytest.mark.parametrize('case', er.WGRAD_EXACT, ids=lambda c: f"s{c[0]}_N{c[1]}_{'x'.join(map(str, c[2]))}_{c[3]}+{c[4]}to{c[5]}+{c[6]}_thr{c[7]}_sl{int(c[8])}")
def test_normalised_wgrad_rounding_within_the_derived_bound(case):
    _ok(gc.check_wgrad_exact(*case))
