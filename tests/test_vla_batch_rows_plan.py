"""Host-side pieces of `VLATrainer(batch_rows=True)`: the grouping of a step's samples, the sample-major row map, and the two new entry points'
prototypes in the header and in the ctypes table.  No GPU."""
import os
import re
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n,max_batch', [(1, 32), (2, 32), (32, 32), (33, 32), (65, 32), (3, 2)])
def test_plan_row_groups(n, max_batch):
    from vlaser_amd.vla_train import plan_row_groups
    groups = plan_row_groups(n, max_batch)
    assert len(groups) == -(-n // max_batch)
    nxt = 0
    for lo, hi, w in groups:
        assert lo == nxt and lo < hi <= n, 'groups must be contiguous and non-empty'
        assert hi - lo <= max_batch
        assert w == (hi - lo) / n
        nxt = hi
    assert nxt == n, 'every sample exactly once'
    assert sum(Fraction(hi - lo, n) for lo, hi, _ in groups) == 1
    assert abs(sum(w for _, _, w in groups) - 1.0) < 1e-12


def test_plan_row_groups_refuses_nonsense():
    from vlaser_amd.vla_train import plan_row_groups
    for n, mb in ((0, 32), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            plan_row_groups(n, mb)


@pytest.mark.parametrize('B,R', [(1, 5), (3, 5), (32, 5), (4, 2), (2, 16)])
def test_expert_row_is_a_bijection(B, R):
    from vlaser_amd.vla_train import expert_row
    rows = [expert_row(b, r, R) for b in range(B) for r in range(R)]
    assert sorted(rows) == list(range(B * R))
    assert rows == list(range(B * R)), 'sample-major: the rows of one sample are adjacent, the proprio token first'


def _n_args(text):
    return len([a for a in text.split(',') if a.strip()])


@pytest.mark.parametrize('name', ['vlaser_attn_rows_bwd_batched', 'vlaser_vla_prep_rows'])
def test_new_prototypes_declared_and_mirrored(name):
    from vlaser_amd import _lib
    h = open(os.path.join(ROOT, 'include', 'vlaser_hip.h')).read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', h, flags=re.S)
    assert m, f'{name} is not declared in include/vlaser_hip.h'
    assert name in _lib._SIGS, f'{name} has no ctypes signature in vlaser_amd/_lib.py'
    assert _n_args(m.group(1)) == len(_lib._SIGS[name]), (name, _n_args(m.group(1)), len(_lib._SIGS[name]))
    from vlaser_amd import ops
    assert hasattr(ops, name[len('vlaser_'):])


def test_constructor_keywords_exist():
    import inspect
    from vlaser_amd.vla_train import VLATrainer
    sig = inspect.signature(VLATrainer.__init__)
    assert sig.parameters['batch_rows'].default is False and sig.parameters['max_batch'].default == 32
    assert hasattr(VLATrainer, 'forward_backward_batch')
