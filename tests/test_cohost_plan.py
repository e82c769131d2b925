"""The pairing of the co-hosted joint prefill (pizero.cohost_plan) on fake launch lists: a pure function of the two lists, no GPU."""
import itertools

import pytest

from vlaser_amd.pizero import COHOST_PAIRS, cohost_plan

HOST_LAYER = ['qkv', 'attn', 'o', 'seam_o', 'gu', 'down', 'seam_d']
GUEST_LAYER = ['qkv', 'attn', 'o', 'gu', 'down']


def lists(n_layers):
    hosts = [(l, n) for l in range(n_layers) for n in (HOST_LAYER if l < n_layers - 1 else ['qkv'])]      # the last VLM layer stops after its q/k/v GEMM
    guests = [(l, n) for l in range(n_layers) for n in GUEST_LAYER]
    return hosts, guests


SUBSETS = [c for r in range(6) for c in itertools.combinations(GUEST_LAYER, r)]


@pytest.mark.parametrize('n_layers', [1, 2, 3, 28])
@pytest.mark.parametrize('enabled', SUBSETS, ids=lambda c: '+'.join(c) or 'none')
def test_plan_invariants(n_layers, enabled):
    hosts, guests = lists(n_layers)
    plan = cohost_plan(hosts, guests, enabled)
    # nothing dropped, nothing doubled, both lists in their own order
    assert [h for h, _ in plan if h is not None] == hosts
    assert [g for _, g in plan if g is not None] == guests
    assert all(h is not None or g is not None for h, g in plan)
    pos_host = {h: i for i, (h, _) in enumerate(plan) if h is not None}
    for i, (h, g) in enumerate(plan):
        if g is None:
            continue
        gl, gn = g
        # every guest sits behind the q/k/v GEMM of its own layer (never in it: that launch writes the prefix keys the guests read)
        assert pos_host[(gl, 'qkv')] < i
        want = (gl, COHOST_PAIRS[gn])
        if h is not None:
            # a hosted guest rides in the launch its pair names, of its own layer, and only when the pair is on
            assert h == want and gn in enabled
        elif want in pos_host:
            # an un-hosted guest whose host exists: its pair is off, and it runs behind that host
            assert gn not in enabled and pos_host[want] < i
        else:
            assert gl == n_layers - 1          # the expert's last layer: no host launches left


def test_all_pairs_on_three_layers():
    hosts, guests = lists(3)
    plan = cohost_plan(hosts, guests)
    # hosted layers: one entry per host launch, five of them carrying a guest
    for l in range(2):
        assert [(h[1], g and g[1]) for h, g in plan if h is not None and h[0] == l] == [
            ('qkv', None), ('attn', 'qkv'), ('o', 'attn'), ('seam_o', 'o'), ('gu', 'gu'), ('down', None), ('seam_d', 'down')]
    # the hand-over: the last VLM layer's q/k/v GEMM alone, then the expert's last layer un-hosted and in order
    assert plan[-6:] == [((2, 'qkv'), None)] + [(None, (2, n)) for n in GUEST_LAYER]


def test_disabled_pair_runs_directly_behind_its_host():
    hosts, guests = lists(2)
    plan = cohost_plan(hosts, guests, ('qkv', 'attn', 'o', 'down'))
    i = plan.index(((0, 'gu'), None))
    assert plan[i + 1] == (None, (0, 'gu'))
    assert plan[i + 2] == ((0, 'down'), None) and plan[i + 3] == ((0, 'seam_d'), (0, 'down'))


def test_pairs_off_is_prefill_interleaved_with_the_expert_in_order():
    hosts, guests = lists(2)
    plan = cohost_plan(hosts, guests, ())
    assert all(h is None or g is None for h, g in plan)
    assert len(plan) == len(hosts) + len(guests)


def test_foreign_launch_names_stay_unhosted():
    """A stack off the chain path has launches under other names (none has a pair): they all come out, in order, each layer's behind its q/k/v GEMM."""
    hosts, _ = lists(3)
    guests = [(l, n) for l in range(3) for n in ('qkv', 'attn_skinny', 'o', 'gu', 'down_partial')]
    plan = cohost_plan(hosts, guests)
    assert [h for h, _ in plan if h is not None] == hosts
    assert [g for _, g in plan if g is not None] == guests
    pos_host = {h: i for i, (h, _) in enumerate(plan) if h is not None}
    for i, (h, g) in enumerate(plan):
        if g is not None:
            assert pos_host[(g[0], 'qkv')] < i
            assert h is None or g[1] in COHOST_PAIRS
