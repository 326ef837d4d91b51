"""dpot_gemm_f32 on the MI355X, descriptor by descriptor: every case of tests/gemm_desc_ref.py CASES - every precision, tile,
operand layout, loader (16-byte / scalar, and each reason for the scalar one), tile epilogue (vector / scalar, each reason),
split-K with its workspace reduce and empty splits, fused column sums, and the hand-off of eligible weight gradients to
gemm_tn_kernel next to ineligible neighbours - against the float64 restatement of the header's epilogue.

Integer operands: no tolerance, torch.equal (gemm_desc_ref explains why all three precisions must give the same bits).  The
Gaussian family (gelu, gelu') is compared with helpers.assert_close at its defaults.  Buffers carry sentinels in every float the
descriptor does not address (pad columns, batch gaps, the floats before a misaligned base): check() finds an overwritten one,
tests/guard.py the writes outside a buffer, and the NaN-poisoned split-K workspace a partial that was never written.  Split-K
cases run twice and must repeat bit for bit (the determinism the header promises)."""
import pytest
import torch

import gemm_desc_ref as R
import guard
from guard import guarded  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ITEMS = R.items()


@pytest.fixture(scope="module")
def ops():
    from dpot_amd import ops as _ops
    from dpot_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(autouse=True)
def _guard(guarded):
    """guarded, poisoned allocations (tests/guard.py): the test's uploads and the split-K workspace ops.gemm allocates"""
    yield guarded


def launch(ops, c, host):
    """upload the buffers of build() (a misaligned base: the view `off` floats into a 512-byte aligned guarded buffer), run
    the descriptor, download everything"""
    dev = {k: guard.wrap(v, "cuda") for k, v in host.items()}
    view = {k: t[c.opnd[k].off:] for k, t in dev.items()}
    for k, t in view.items():
        assert t.data_ptr() % 16 == 4 * c.opnd[k].off, f"{c.label}: {k} is not at base + {c.opnd[k].off} floats"
    ops.gemm(view["A"], view["B"], view["C"], c.M, c.N, c.K, bias=view.get("bias"), aux=view.get("aux"),
             preact=view.get("preact"), res=view.get("res"), colsum_out=view.get("colsum"), **R.gemm_kwargs(c))
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def run_case(ops, c):
    host = R.build(c, R.seed_of(c))
    ref = R.reference(c, host)
    first = launch(ops, c, host)
    R.check(c, host, first, ref)
    if c.splitk > 1:
        again = launch(ops, c, host)
        R.check(c, host, again, ref)
        for name in R.OUTPUTS:
            if c.has(name):
                idx = c.opnd[name].index(c.batch)
                assert torch.equal(first[name][idx], again[name][idx]), f"{c.label}: {name} differs between two runs"


@pytest.mark.parametrize("item", sorted(ITEMS))
def test_descriptors_equal_the_float64_reference(ops, item):
    failed = []
    for c in ITEMS[item]:
        try:
            run_case(ops, c)
        except AssertionError as e:          # a wrong result: go on, report every failing case of the item
            failed.append(str(e))            # (anything else - a HIP error - ends the item at once)
    print(f"{item}: {len(ITEMS[item])} cases, {len(failed)} failed")
    assert not failed, f"{len(failed)} of {len(ITEMS[item])} cases of {item} failed:\n" + "\n".join(failed[:20])


def test_items_are_the_table():
    ran = [c.label for cases in ITEMS.values() for c in cases]
    assert sorted(ran) == sorted(c.label for c in R.CASES) and len(set(ran)) == len(ran) == len(R.CASES)
