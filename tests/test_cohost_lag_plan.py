"""The lagged pairing of the co-hosted joint prefill (pizero.cohost_plan(..., lagged=('down',)): the expert's down projection of layer l rides in the q/k/v GEMM of VLM
layer l + 1) on fake launch lists: a pure function of the two lists, no GPU."""
import itertools

import pytest

from vlaser_amd.pizero import COHOST_LAGGED, COHOST_PAIRS, cohost_plan

HOST_LAYER = ['qkv', 'attn', 'o', 'seam_o', 'gu', 'down', 'seam_d']
GUEST_LAYER = ['qkv', 'attn', 'o', 'gu', 'down']
SUBSETS = [c for r in range(6) for c in itertools.combinations(GUEST_LAYER, r)]
LAYERS = [1, 2, 3, 28]


def lists(n_layers):
    hosts = [(l, n) for l in range(n_layers) for n in (HOST_LAYER if l < n_layers - 1 else ['qkv'])]      # the last VLM layer stops after its q/k/v GEMM
    guests = [(l, n) for l in range(n_layers) for n in GUEST_LAYER]
    return hosts, guests


def todays_plan(hosts, guests, enabled):
    """The un-lagged plan written out from its rules, independently of cohost_plan: walk the hosts; a guest whose pair is on and whose host this is rides; then every
    guest in order whose place (its host, or its layer's q/k/v GEMM where that host does not exist) has been issued runs on its own."""
    place = lambda g: (g[0], COHOST_PAIRS[g[1]]) if (g[0], COHOST_PAIRS[g[1]]) in hosts else (g[0], 'qkv')
    out, rest = [], list(guests)
    for hi, h in enumerate(hosts):
        rides = bool(rest) and rest[0][1] in enabled and (rest[0][0], COHOST_PAIRS[rest[0][1]]) == h
        out.append((h, rest.pop(0) if rides else None))
        while rest and hosts.index(place(rest[0])) <= hi:
            out.append((None, rest.pop(0)))
    assert not rest
    return out


def test_the_table():
    assert COHOST_LAGGED == {'down': 'qkv'}


@pytest.mark.parametrize('n_layers', LAYERS)
@pytest.mark.parametrize('enabled', SUBSETS, ids=lambda c: '+'.join(c) or 'none')
def test_lagged_plan_invariants(n_layers, enabled):
    hosts, guests = lists(n_layers)
    plan = cohost_plan(hosts, guests, enabled, lagged=('down',))
    # nothing dropped, nothing doubled, both lists in their own order
    assert [h for h, _ in plan if h is not None] == hosts
    assert [g for _, g in plan if g is not None] == guests
    assert all(h is not None or g is not None for h, g in plan)
    pos_host = {h: i for i, (h, _) in enumerate(plan) if h is not None}
    for i, (h, g) in enumerate(plan):
        if g is None:
            continue
        gl, gn = g
        # every guest sits behind the q/k/v GEMM of its own layer
        assert pos_host[(gl, 'qkv')] < i
        if gn == 'down' and gl < n_layers - 1:
            # d(l) rides in the q/k/v GEMM of layer l + 1, whether or not its own pair is on, and never elsewhere
            assert h == (gl + 1, 'qkv')
            continue
        assert h is None or h[1] != 'qkv', 'the q/k/v GEMM carries the lagged down projection only'
        want = (gl, COHOST_PAIRS[gn])
        if h is not None:
            assert h == want and gn in enabled
        elif want in pos_host:
            assert gn not in enabled and pos_host[want] < i
        else:
            assert gl == n_layers - 1          # the expert's last layer: no host launches left
    # every q/k/v GEMM but the first carries the previous layer's down projection
    assert [g for h, g in plan if h is not None and h[1] == 'qkv'] == [None] + [(l, 'down') for l in range(n_layers - 1)]


@pytest.mark.parametrize('n_layers', LAYERS)
@pytest.mark.parametrize('enabled', SUBSETS, ids=lambda c: '+'.join(c) or 'none')
def test_no_lag_is_todays_plan(n_layers, enabled):
    hosts, guests = lists(n_layers)
    want = todays_plan(hosts, guests, enabled)
    assert cohost_plan(hosts, guests, enabled, lagged=()) == want
    assert cohost_plan(hosts, guests, enabled) == want


def test_three_layers_spelled_out():
    hosts, guests = lists(3)
    plan = cohost_plan(hosts, guests, ('qkv', 'attn', 'o', 'gu'), lagged=('down',))
    assert plan == [
        ((0, 'qkv'), None), ((0, 'attn'), (0, 'qkv')), ((0, 'o'), (0, 'attn')), ((0, 'seam_o'), (0, 'o')), ((0, 'gu'), (0, 'gu')), ((0, 'down'), None), ((0, 'seam_d'), None),
        ((1, 'qkv'), (0, 'down')), ((1, 'attn'), (1, 'qkv')), ((1, 'o'), (1, 'attn')), ((1, 'seam_o'), (1, 'o')), ((1, 'gu'), (1, 'gu')), ((1, 'down'), None), ((1, 'seam_d'), None),
        # the hand-over: the last VLM layer's q/k/v GEMM carries d(1); the expert's last layer un-hosted and in order
        ((2, 'qkv'), (1, 'down')), (None, (2, 'qkv')), (None, (2, 'attn')), (None, (2, 'o')), (None, (2, 'gu')), (None, (2, 'down'))]
    # the lag alone: every other guest directly behind its host, the down projection still one layer later
    alone = cohost_plan(hosts, guests, (), lagged=('down',))
    assert alone[:13] == [
        ((0, 'qkv'), None), ((0, 'attn'), None), (None, (0, 'qkv')), ((0, 'o'), None), (None, (0, 'attn')), ((0, 'seam_o'), None), (None, (0, 'o')), ((0, 'gu'), None),
        (None, (0, 'gu')), ((0, 'down'), None), ((0, 'seam_d'), None), ((1, 'qkv'), (0, 'down')), ((1, 'attn'), None)]


def test_one_layer_has_nothing_to_lag():
    hosts, guests = lists(1)
    assert cohost_plan(hosts, guests, lagged=('down',)) == [((0, 'qkv'), None)] + [(None, g) for g in guests]


def test_option_tokens():
    """'down_next' among the pairs of the Euler option: parsed without a GPU by the function PiZero.__init__ calls (pizero.resolve_euler_opts; tests/test_euler_opts.py)."""
    from vlaser_amd.pizero import LAG_TOKENS, resolve_euler_opts
    assert resolve_euler_opts('qkv16,gu16,glue1,chain,cohost=qkv+down_next')[2:] == (('qkv',), ('down',))
    assert LAG_TOKENS == {'down_next': 'down'} and all(v in COHOST_LAGGED for v in LAG_TOKENS.values())
