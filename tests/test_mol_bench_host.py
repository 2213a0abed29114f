"""CPU: the molecule timing tools (tools/bench_mol_*.py, bench_fingerprints.py, bench_shape.py, bench_shape_align.py) and the module
they share, tools/mol_bench.py.  Every tool imports without a GPU and without the library and exposes `main`; the synthetic inputs
of mol_bench.py come out in the sampler's layout."""
import importlib
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if TOOLS not in sys.path:
    sys.path.append(TOOLS)
import mol_bench as mb  # noqa: E402
from phoregen_amd.plan import make_edge_data  # noqa: E402

TOOL_NAMES = ['bench_mol_' + k for k in ('screen', 'key', 'geom', 'rings', 'kekule', 'feat', 'smiles', 'stereo', 'hydrogens', 'scaffold',
                                         'props', 'sub')] + ['bench_fingerprints', 'bench_shape', 'bench_shape_align']


@pytest.mark.parametrize('name', TOOL_NAMES)
def test_every_tool_imports_and_exposes_main(name):
    assert callable(importlib.import_module(name).main)


RESULTS = [('dense_result', lambda: mb.dense_result(2, 5, 'cpu'), [5, 5]),
           ('onehot_result of (1, 3, 2 atoms)', lambda: mb.onehot_result([([1], {}), ([1, 2, 3], {(0, 1): 1, (1, 2): 2}), ([1, 1], {(0, 1): 4})], 'cpu'),
            [1, 3, 2]),
           ('onehot_result of 2 ladders', lambda: mb.onehot_result(mb.ladder_graphs(2, 6), 'cpu'), [6, 6]),
           ('onehot_result of 2 label chains', lambda: mb.onehot_result(mb.label_chain_graphs(2, 8, closures=2), 'cpu'), [8, 8]),
           ('onehot_result of 2 sparse aromatic graphs', lambda: mb.onehot_result(mb.sparse_aromatic_graphs(2, n=33), 'cpu'), [33, 33]),
           ('chain_result', lambda: mb.chain_result(2, 4, 'cpu'), [4, 4]),
           ('molecule_like', lambda: mb.molecule_like([3, 1, 5], 'cpu'), [3, 1, 5])]


@pytest.mark.parametrize('label, build, sizes', RESULTS, ids=[r[0] for r in RESULTS])
def test_synthetic_results_have_the_samplers_layout(label, build, sizes):
    res = build()
    node, pos, edge = res['pred']
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    assert node.shape == (N, 12) and pos.shape == (N, 3) and edge.shape == (E, 6)
    assert node.dtype == pos.dtype == edge.dtype == torch.float32 and res['traj'] == [None, None, None]
    na, batch, ei, eb = res['lig_info']
    assert na.tolist() == sizes and int(na.sum()) == N
    assert batch.tolist() == [g for g, n in enumerate(sizes) for _ in range(n)]
    want_ei, want_eb = make_edge_data(torch.tensor(sizes, dtype=torch.long))
    assert torch.equal(ei, want_ei) and torch.equal(eb, want_eb) and ei.size(1) == E


def test_onehot_result_puts_each_bond_in_both_halves_of_its_graphs_rows():
    res = mb.onehot_result([([1, 2, 3], {(0, 2): 2}), ([1, 1], {(0, 1): 4})], 'cpu')
    node, _, edge = res['pred']
    assert node.argmax(1).tolist() == [1, 2, 3, 1, 1] and bool((node.sum(1) == 1).all()) and bool((edge.sum(1) == 1).all())
    # graph 0: 3 pair rows (0,1) (0,2) (1,2), then the same three again; graph 1: its one pair, twice
    assert edge.argmax(1).tolist() == [0, 2, 0, 0, 2, 0, 4, 4]


def test_graph_lists_are_what_their_docstrings_say():
    (classes, bonds), = mb.ladder_graphs(1, 6)
    assert classes == [1] * 6 and bonds == {(0, 1): 4, (1, 2): 4, (3, 4): 4, (4, 5): 4, (0, 3): 4, (2, 5): 4}
    (classes, bonds), = mb.label_chain_graphs(1, 8, closures=2)
    assert classes == [1] * 8 and bonds == {**{(i, i + 1): 1 for i in range(7)}, (0, 2): 1, (0, 3): 1}
    n = 33                                                             # the smallest: 30 ring atoms and one chain atom for each ring pair
    graphs = mb.sparse_aromatic_graphs(2, n=n)
    assert len(graphs) == 2 and graphs == mb.sparse_aromatic_graphs(2, n=n) and graphs[0] != graphs[1]      # seeded; renumbered per graph
    for classes, bonds in graphs:
        degree = [0] * n
        for (a, b), t in bonds.items():
            assert 0 <= a < b < n and t in (1, 4)
            degree[a] += 1
            degree[b] += 1
        # three ring pairs of 10 atoms and 11 aromatic bonds each, a bond from each to the chain of the other 3 atoms
        assert len(classes) == n and set(classes) <= {1, 2} and sorted(bonds.values()) == [1] * 5 + [4] * 33 and max(degree) == 3
    assert len(mb.onehot_result(graphs, 'cpu')['pred'][0]) == 2 * n


def test_chain_result_is_a_chain_with_a_hetero_atom_in_every_fourth_place():
    node, _, edge = mb.chain_result(2, 9, 'cpu')['pred']
    assert node.argmax(1).tolist() == [1, 1, 1, 2, 1, 1, 1, 3, 1] * 2
    h = 36
    first = edge[:h].argmax(1)
    rows = [a * 9 - a * (a + 1) // 2 for a in range(8)]                # the pair (a, a + 1) is the first of row a
    assert first.nonzero().flatten().tolist() == rows and first[rows].tolist() == [1] * 8 and torch.equal(edge[:h], edge[h:2 * h])


def test_fmt_and_report(tmp_path, capsys):
    assert mb.fmt((1.0, 0.5, 2.25)) == '1.000 (0.500 - 2.250)' == mb.fmt((1.0, 0.5, 2.25, 'outputs'))
    out = tmp_path / 't.md'
    text, record = mb.report(['| a |', '|---|'], {'k': 1.5}, str(out))
    assert text == '| a |\n|---|\n' == out.read_text() and record == {'k': 1.5}
    assert capsys.readouterr().out == text + '\n{"k": 1.5}\n'
    args = mb.parser(50).parse_args(['--graphs', '3'])
    assert (args.steps, args.graphs, args.out) == (50, 3, None) and mb.parser().parse_args([]).steps == 1000
