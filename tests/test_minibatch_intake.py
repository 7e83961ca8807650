"""The refusals that the mini-batch ops (pygat_amd/sampling.py, subgraph.py, linkpred.py) make through their shared intake
(pygat_amd/_minibatch.py), word for word: no GPU is needed, a CSRGraph that was never built stands in for the graph (as in
test_linkpred_abi.py) and a CPU tensor that claims to be on the GPU for the ids.  EXPECTED was recorded from the commit before the
intake was shared: the messages are behaviour, and so is the order in which two bad arguments are refused."""
import pytest
import torch


class OnGpu(torch.Tensor):
    is_cuda = property(lambda self: True)


def _gpu(t):
    return t.as_subclass(OnGpu)


def _fake_graph():
    """A CSRGraph that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    g = object.__new__(pg.CSRGraph)
    g.device, g.n, g.nnz = torch.device("cpu"), 10, 30
    return g


IDS = torch.arange(4)
W = torch.ones(30)


def _kw(seed, hop):
    return {k: v for k, v in (("seed", seed), ("hop", hop)) if v is not None}


# op -> (the name of its count argument or None, whether it has seed / hop, call(pg, graph, ids, count, seed, hop))
OPS = {
    "sample_neighbors": ("fanout", True, True, lambda pg, g, t, c, s, h: pg.sample_neighbors(g, t, c, **_kw(s, h))),
    "sample_neighbors_weighted": ("fanout", True, True, lambda pg, g, t, c, s, h: pg.sample_neighbors_weighted(g, t, c, W, **_kw(s, h))),
    "sample_blocks": ("fanout", True, False, lambda pg, g, t, c, s, h: pg.sample_blocks(g, t, [c], **_kw(s, h))),
    "sample_blocks_weighted": ("fanout", True, False, lambda pg, g, t, c, s, h: pg.sample_blocks_weighted(g, t, [c], W, **_kw(s, h))),
    "induced_subgraph": (None, False, False, lambda pg, g, t, c, s, h: pg.induced_subgraph(g, t)),
    "random_walk": ("length", True, True, lambda pg, g, t, c, s, h: pg.random_walk(g, t, c, **_kw(s, h))),
    "find_edges": (None, False, False, lambda pg, g, t, c, s, h: pg.find_edges(g, t, _gpu(IDS))),
    "find_edges.col": (None, False, False, lambda pg, g, t, c, s, h: pg.find_edges(g, _gpu(IDS), t)),
    "negative_edges": ("num_neg", True, True, lambda pg, g, t, c, s, h: pg.negative_edges(g, t, c, **_kw(s, h))),
    "link_batch": ("num_neg", True, False, lambda pg, g, t, c, s, h: pg.link_batch(g, t, c, [10], **_kw(s, h))),
    "link_batch.fanouts": ("fanout", False, False, lambda pg, g, t, c, s, h: pg.link_batch(g, t, 5, [c])),
}


def _cases(op):
    """(case name, graph, ids, count, seed, hop) of every refusal of `op` that the shared intake words."""
    count, has_seed, has_hop, _ = OPS[op]
    g, t = _fake_graph(), _gpu(IDS)
    yield "graph", (IDS, IDS), t, 5, None, None
    yield "ids no tensor", g, [0, 1], 5, None, None
    yield "ids on the cpu", g, IDS, 5, None, None
    yield "ids float", g, _gpu(IDS.float()), 5, None, None
    yield "ids 2-d", g, _gpu(IDS.view(2, 2)), 5, None, None
    yield "ids empty", g, _gpu(IDS[:0]), 5, None, None
    if has_seed:
        yield "seed dtype", g, t, 5, torch.zeros(1, dtype=torch.int32), None
        yield "seed shape", g, t, 5, torch.zeros(2, dtype=torch.int64), None
    if has_hop:
        for bad in (-1, 2 ** 32, True):
            yield f"hop {bad!r}", g, t, 5, None, bad
    if count:
        for bad in (0, True, 1.5):
            yield f"{count} {bad!r}", g, t, bad, None, None


# two bad arguments at once: the one refused first
ORDER = {
    "sample_neighbors: fanout before hop before seed before dst":
        lambda pg: pg.sample_neighbors(_fake_graph(), IDS.float(), 0, seed=7, hop=-1),
    "sample_neighbors: hop before seed before dst": lambda pg: pg.sample_neighbors(_fake_graph(), IDS.float(), 5, seed=7, hop=-1),
    "sample_neighbors: seed before dst": lambda pg: pg.sample_neighbors(_fake_graph(), IDS.float(), 5, seed=7),
    "negative_edges: num_neg before hop before the flags before seed before src":
        lambda pg: pg.negative_edges(_fake_graph(), IDS.float(), 0, seed=7, hop=-1, exclude_self=1),
    "negative_edges: hop before the flags before seed before src":
        lambda pg: pg.negative_edges(_fake_graph(), IDS.float(), 5, seed=7, hop=-1, exclude_self=1),
    "negative_edges: the flags before seed before src": lambda pg: pg.negative_edges(_fake_graph(), IDS.float(), 5, seed=7, exclude_self=1),
    "negative_edges: seed before src": lambda pg: pg.negative_edges(_fake_graph(), IDS.float(), 5, seed=7),
}


def _refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


EXPECTED = {'sample_neighbors': {'graph': 'pygat_amd sample_neighbors: a CSRGraph expected, not tuple',
                      'ids no tensor': 'pygat_amd sample_neighbors: dst must be a tensor on the GPU (there is no CPU path)',
                      'ids on the cpu': 'pygat_amd sample_neighbors: dst must be a tensor on the GPU (there is no CPU path)',
                      'ids float': 'pygat_amd sample_neighbors: dst must be int32 or int64, not torch.float32',
                      'ids 2-d': 'pygat_amd sample_neighbors: dst [n_dst] with n_dst >= 1 expected, got (2, 2)',
                      'ids empty': 'pygat_amd sample_neighbors: dst [n_dst] with n_dst >= 1 expected, got (0,)',
                      'seed dtype': "pygat_amd sample_neighbors: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels "
                                    'read it there), got torch.int32 (1,) on cpu',
                      'seed shape': "pygat_amd sample_neighbors: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels "
                                    'read it there), got torch.int64 (2,) on cpu',
                      'hop -1': 'pygat_amd sample_neighbors: hop = -1: an int in [0, 2^32) expected',
                      'hop 4294967296': 'pygat_amd sample_neighbors: hop = 4294967296: an int in [0, 2^32) expected',
                      'hop True': 'pygat_amd sample_neighbors: hop = True: an int in [0, 2^32) expected',
                      'fanout 0': 'pygat_amd sample_neighbors: fanout = 0: an int >= 1, or None for whole rows, expected',
                      'fanout True': 'pygat_amd sample_neighbors: fanout = True: an int >= 1, or None for whole rows, expected',
                      'fanout 1.5': 'pygat_amd sample_neighbors: fanout = 1.5: an int >= 1, or None for whole rows, expected'},
 'sample_neighbors_weighted': {'graph': 'pygat_amd sample_neighbors_weighted: a CSRGraph expected, not tuple',
                               'ids no tensor': 'pygat_amd sample_neighbors_weighted: dst must be a tensor on the GPU (there is no CPU path)',
                               'ids on the cpu': 'pygat_amd sample_neighbors_weighted: dst must be a tensor on the GPU (there is no CPU path)',
                               'ids float': 'pygat_amd sample_neighbors_weighted: dst must be int32 or int64, not torch.float32',
                               'ids 2-d': 'pygat_amd sample_neighbors_weighted: dst [n_dst] with n_dst >= 1 expected, got (2, 2)',
                               'ids empty': 'pygat_amd sample_neighbors_weighted: dst [n_dst] with n_dst >= 1 expected, got (0,)',
                               'seed dtype': "pygat_amd sample_neighbors_weighted: seed must be an int64 tensor of shape [1] on the graph's device "
                                             'cpu (the kernels read it there), got torch.int32 (1,) on cpu',
                               'seed shape': "pygat_amd sample_neighbors_weighted: seed must be an int64 tensor of shape [1] on the graph's device "
                                             'cpu (the kernels read it there), got torch.int64 (2,) on cpu',
                               'hop -1': 'pygat_amd sample_neighbors_weighted: hop = -1: an int in [0, 2^32) expected',
                               'hop 4294967296': 'pygat_amd sample_neighbors_weighted: hop = 4294967296: an int in [0, 2^32) expected',
                               'hop True': 'pygat_amd sample_neighbors_weighted: hop = True: an int in [0, 2^32) expected',
                               'fanout 0': 'pygat_amd sample_neighbors_weighted: fanout = 0: an int >= 1, or None for whole rows, expected',
                               'fanout True': 'pygat_amd sample_neighbors_weighted: fanout = True: an int >= 1, or None for whole rows, expected',
                               'fanout 1.5': 'pygat_amd sample_neighbors_weighted: fanout = 1.5: an int >= 1, or None for whole rows, expected'},
 'sample_blocks': {'graph': 'pygat_amd sample_blocks: a CSRGraph expected, not tuple',
                   'ids no tensor': 'pygat_amd sample_blocks: dst must be a tensor on the GPU (there is no CPU path)',
                   'ids on the cpu': 'pygat_amd sample_blocks: dst must be a tensor on the GPU (there is no CPU path)',
                   'ids float': 'pygat_amd sample_blocks: dst must be int32 or int64, not torch.float32',
                   'ids 2-d': 'pygat_amd sample_blocks: dst [n_dst] with n_dst >= 1 expected, got (2, 2)',
                   'ids empty': 'pygat_amd sample_blocks: dst [n_dst] with n_dst >= 1 expected, got (0,)',
                   'seed dtype': "pygat_amd sample_blocks: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                                 'there), got torch.int32 (1,) on cpu',
                   'seed shape': "pygat_amd sample_blocks: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                                 'there), got torch.int64 (2,) on cpu',
                   'fanout 0': 'pygat_amd sample_blocks: fanout = 0: an int >= 1, or None for whole rows, expected',
                   'fanout True': 'pygat_amd sample_blocks: fanout = True: an int >= 1, or None for whole rows, expected',
                   'fanout 1.5': 'pygat_amd sample_blocks: fanout = 1.5: an int >= 1, or None for whole rows, expected'},
 'sample_blocks_weighted': {'graph': 'pygat_amd sample_blocks_weighted: a CSRGraph expected, not tuple',
                            'ids no tensor': 'pygat_amd sample_blocks_weighted: dst must be a tensor on the GPU (there is no CPU path)',
                            'ids on the cpu': 'pygat_amd sample_blocks_weighted: dst must be a tensor on the GPU (there is no CPU path)',
                            'ids float': 'pygat_amd sample_blocks_weighted: dst must be int32 or int64, not torch.float32',
                            'ids 2-d': 'pygat_amd sample_blocks_weighted: dst [n_dst] with n_dst >= 1 expected, got (2, 2)',
                            'ids empty': 'pygat_amd sample_blocks_weighted: dst [n_dst] with n_dst >= 1 expected, got (0,)',
                            'seed dtype': "pygat_amd sample_blocks_weighted: seed must be an int64 tensor of shape [1] on the graph's device cpu "
                                          '(the kernels read it there), got torch.int32 (1,) on cpu',
                            'seed shape': "pygat_amd sample_blocks_weighted: seed must be an int64 tensor of shape [1] on the graph's device cpu "
                                          '(the kernels read it there), got torch.int64 (2,) on cpu',
                            'fanout 0': 'pygat_amd sample_blocks_weighted: fanout = 0: an int >= 1, or None for whole rows, expected',
                            'fanout True': 'pygat_amd sample_blocks_weighted: fanout = True: an int >= 1, or None for whole rows, expected',
                            'fanout 1.5': 'pygat_amd sample_blocks_weighted: fanout = 1.5: an int >= 1, or None for whole rows, expected'},
 'induced_subgraph': {'graph': 'pygat_amd induced_subgraph: a CSRGraph expected, not tuple',
                      'ids no tensor': 'pygat_amd induced_subgraph: nodes must be a tensor on the GPU (there is no CPU path)',
                      'ids on the cpu': 'pygat_amd induced_subgraph: nodes must be a tensor on the GPU (there is no CPU path)',
                      'ids float': 'pygat_amd induced_subgraph: nodes must be int32 or int64, not torch.float32',
                      'ids 2-d': 'pygat_amd induced_subgraph: nodes [n_in] with n_in >= 1 expected, got (2, 2)',
                      'ids empty': 'pygat_amd induced_subgraph: nodes [n_in] with n_in >= 1 expected, got (0,)'},
 'random_walk': {'graph': 'pygat_amd random_walk: a CSRGraph expected, not tuple',
                 'ids no tensor': 'pygat_amd random_walk: start must be a tensor on the GPU (there is no CPU path)',
                 'ids on the cpu': 'pygat_amd random_walk: start must be a tensor on the GPU (there is no CPU path)',
                 'ids float': 'pygat_amd random_walk: start must be int32 or int64, not torch.float32',
                 'ids 2-d': 'pygat_amd random_walk: start [n_walk] with n_walk >= 1 expected, got (2, 2)',
                 'ids empty': 'pygat_amd random_walk: start [n_walk] with n_walk >= 1 expected, got (0,)',
                 'seed dtype': "pygat_amd random_walk: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                               'there), got torch.int32 (1,) on cpu',
                 'seed shape': "pygat_amd random_walk: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                               'there), got torch.int64 (2,) on cpu',
                 'hop -1': 'pygat_amd random_walk: hop = -1: an int in [0, 2^32) expected',
                 'hop 4294967296': 'pygat_amd random_walk: hop = 4294967296: an int in [0, 2^32) expected',
                 'hop True': 'pygat_amd random_walk: hop = True: an int in [0, 2^32) expected',
                 'length 0': 'pygat_amd random_walk: length = 0: an int >= 1 expected',
                 'length True': 'pygat_amd random_walk: length = True: an int >= 1 expected',
                 'length 1.5': 'pygat_amd random_walk: length = 1.5: an int >= 1 expected'},
 'find_edges': {'graph': 'pygat_amd find_edges: a CSRGraph expected, not tuple',
                'ids no tensor': 'pygat_amd find_edges: row must be a tensor on the GPU (there is no CPU path)',
                'ids on the cpu': 'pygat_amd find_edges: row must be a tensor on the GPU (there is no CPU path)',
                'ids float': 'pygat_amd find_edges: row must be int32 or int64, not torch.float32',
                'ids 2-d': 'pygat_amd find_edges: row [n] with n >= 1 expected, got (2, 2)',
                'ids empty': 'pygat_amd find_edges: row [n] with n >= 1 expected, got (0,)'},
 'find_edges.col': {'graph': 'pygat_amd find_edges: a CSRGraph expected, not tuple',
                    'ids no tensor': 'pygat_amd find_edges: col must be a tensor on the GPU (there is no CPU path)',
                    'ids on the cpu': 'pygat_amd find_edges: col must be a tensor on the GPU (there is no CPU path)',
                    'ids float': 'pygat_amd find_edges: col must be int32 or int64, not torch.float32',
                    'ids 2-d': 'pygat_amd find_edges: col [n] with n >= 1 expected, got (2, 2)',
                    'ids empty': 'pygat_amd find_edges: col [n] with n >= 1 expected, got (0,)'},
 'negative_edges': {'graph': 'pygat_amd negative_edges: a CSRGraph expected, not tuple',
                    'ids no tensor': 'pygat_amd negative_edges: src must be a tensor on the GPU (there is no CPU path)',
                    'ids on the cpu': 'pygat_amd negative_edges: src must be a tensor on the GPU (there is no CPU path)',
                    'ids float': 'pygat_amd negative_edges: src must be int32 or int64, not torch.float32',
                    'ids 2-d': 'pygat_amd negative_edges: src [n_src] with n_src >= 1 expected, got (2, 2)',
                    'ids empty': 'pygat_amd negative_edges: src [n_src] with n_src >= 1 expected, got (0,)',
                    'seed dtype': "pygat_amd negative_edges: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read "
                                  'it there), got torch.int32 (1,) on cpu',
                    'seed shape': "pygat_amd negative_edges: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read "
                                  'it there), got torch.int64 (2,) on cpu',
                    'hop -1': 'pygat_amd negative_edges: hop = -1: an int in [0, 2^32) expected',
                    'hop 4294967296': 'pygat_amd negative_edges: hop = 4294967296: an int in [0, 2^32) expected',
                    'hop True': 'pygat_amd negative_edges: hop = True: an int in [0, 2^32) expected',
                    'num_neg 0': 'pygat_amd negative_edges: num_neg = 0: an int >= 1 expected',
                    'num_neg True': 'pygat_amd negative_edges: num_neg = True: an int >= 1 expected',
                    'num_neg 1.5': 'pygat_amd negative_edges: num_neg = 1.5: an int >= 1 expected'},
 'link_batch': {'graph': 'pygat_amd link_batch: a CSRGraph expected, not tuple',
                'ids no tensor': 'pygat_amd link_batch: edge_ids must be a tensor on the GPU (there is no CPU path)',
                'ids on the cpu': 'pygat_amd link_batch: edge_ids must be a tensor on the GPU (there is no CPU path)',
                'ids float': 'pygat_amd link_batch: edge_ids must be int32 or int64, not torch.float32',
                'ids 2-d': 'pygat_amd link_batch: edge_ids [B] with B >= 1 expected, got (2, 2)',
                'ids empty': 'pygat_amd link_batch: edge_ids [B] with B >= 1 expected, got (0,)',
                'seed dtype': "pygat_amd link_batch: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                              'there), got torch.int32 (1,) on cpu',
                'seed shape': "pygat_amd link_batch: seed must be an int64 tensor of shape [1] on the graph's device cpu (the kernels read it "
                              'there), got torch.int64 (2,) on cpu',
                'num_neg 0': 'pygat_amd link_batch: num_neg = 0: an int >= 1 expected',
                'num_neg True': 'pygat_amd link_batch: num_neg = True: an int >= 1 expected',
                'num_neg 1.5': 'pygat_amd link_batch: num_neg = 1.5: an int >= 1 expected'},
 'link_batch.fanouts': {'graph': 'pygat_amd link_batch: a CSRGraph expected, not tuple',
                        'ids no tensor': 'pygat_amd link_batch: edge_ids must be a tensor on the GPU (there is no CPU path)',
                        'ids on the cpu': 'pygat_amd link_batch: edge_ids must be a tensor on the GPU (there is no CPU path)',
                        'ids float': 'pygat_amd link_batch: edge_ids must be int32 or int64, not torch.float32',
                        'ids 2-d': 'pygat_amd link_batch: edge_ids [B] with B >= 1 expected, got (2, 2)',
                        'ids empty': 'pygat_amd link_batch: edge_ids [B] with B >= 1 expected, got (0,)',
                        'fanout 0': 'pygat_amd link_batch: fanout = 0: an int >= 1, or None for whole rows, expected',
                        'fanout True': 'pygat_amd link_batch: fanout = True: an int >= 1, or None for whole rows, expected',
                        'fanout 1.5': 'pygat_amd link_batch: fanout = 1.5: an int >= 1, or None for whole rows, expected'},
 'order': {'sample_neighbors: fanout before hop before seed before dst': 'pygat_amd sample_neighbors: fanout = 0: an int >= 1, or None for whole '
                                                                         'rows, expected',
           'sample_neighbors: hop before seed before dst': 'pygat_amd sample_neighbors: hop = -1: an int in [0, 2^32) expected',
           'sample_neighbors: seed before dst': "pygat_amd sample_neighbors: seed must be an int64 tensor of shape [1] on the graph's device cpu "
                                                '(the kernels read it there), got int',
           'negative_edges: num_neg before hop before the flags before seed before src': 'pygat_amd negative_edges: num_neg = 0: an int >= 1 '
                                                                                         'expected',
           'negative_edges: hop before the flags before seed before src': 'pygat_amd negative_edges: hop = -1: an int in [0, 2^32) expected',
           'negative_edges: the flags before seed before src': 'pygat_amd negative_edges: exclude_self = 1: True or False expected',
           'negative_edges: seed before src': "pygat_amd negative_edges: seed must be an int64 tensor of shape [1] on the graph's device cpu (the "
                                              'kernels read it there), got int'}}


@pytest.mark.parametrize("op", list(OPS))
def test_every_shared_refusal_word_for_word(op):
    import pygat_amd as pg
    call = OPS[op][3]
    cases = list(_cases(op))
    assert [name for name, *_ in cases] == list(EXPECTED[op]), op
    for name, *args in cases:
        assert _refusal(lambda: call(pg, *args)) == EXPECTED[op][name], (op, name)


@pytest.mark.parametrize("case", list(ORDER))
def test_the_order_of_two_refusals(case):
    import pygat_amd as pg
    assert _refusal(lambda: ORDER[case](pg)) == EXPECTED["order"][case], case
