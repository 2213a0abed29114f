"""-m gpu: every molecule timing tool runs end to end, in-process, at toy size.  Three ragged graphs of the bench workload and two
reverse steps are the smallest input that still has different atom counts per graph and a trajectory of several frames (3).  What is
checked is the instrument, not a time: the table has its header and one row per case, every timing of the record is finite and
positive, and a second run gives the same record keys.  The equality asserts of `mol_bench.relaunch_ms` (and the tools' own) run on
the way: they are what notices a `_launch_X` call in a tool that no longer matches the public function."""
import importlib
import math
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if TOOLS not in sys.path:
    sys.path.append(TOOLS)

pytestmark = pytest.mark.gpu
TOY = ['--graphs', '3', '--steps', '2']
AB = ['| (a) final frame, 3 graphs |', '| (b) trajectory, 3 frames x 3 graphs, ONE launch |']
SUB_ROWS = ['| 1 |', '| 16 |', '| 256 |']

# tool: (arguments, what the text must hold: header cells, then the start of every row)
CASES = {
    'bench_mol_screen': (TOY + ['--tile', '2'], ['| case | kernel ms, median (min - max) | GB/s of needed traffic |', AB[0], AB[1], '| (c) final frame, 6 graphs |']),
    'bench_mol_key': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_key` kernel ms | key / screen |'] + AB),
    'bench_mol_geom': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_geom` kernel ms | geom / screen |'] + AB),
    'bench_mol_rings': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_rings` kernel ms | rings / screen |'] + AB
                        + ['| (c) worst case: 3 graphs of 128 atoms, random logits (dense) |']),
    'bench_mol_kekule': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_kekule` kernel ms | kekule / screen |'] + AB
                         + ['| (c) sparse aromatic: 3 graphs of 64 atoms, 30 aromatic |', '| (d) serial worst case: 3 ladders of 128 aromatic C |']),
    'bench_mol_feat': (TOY + ['--repeats', '2'], ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_geom` kernel ms | `pg_mol_feat` kernel ms | feat / geom |',
                                                  '| (a) final frame, 3 graphs, their ', '| (b) sparse aromatic: 3 graphs of 64 atoms, 12 points each on their atoms |']),
    'bench_mol_smiles': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_kekule` kernel ms | `pg_mol_smiles` kernel ms | smiles / screen |'] + AB
                         + ['| (c) sparse aromatic: 3 graphs of 64 atoms, 30 aromatic |', '| (d) longest walk: 3 chains of 128 C with 99 closures open at once |']),
    'bench_mol_stereo': (TOY, ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_smiles` kernel ms | `pg_mol_stereo` kernel ms | '
                               '`pg_mol_smiles_stereo` kernel ms | stereo / screen |'] + AB),
    'bench_mol_hydrogens': (TOY, ['| case | `pg_mol_stereo` kernel ms, median (min - max) | `pg_mol_hydrogens` kernel ms | hydrogens / stereo |',
                                  '| (a) final frame, 1 frames x 3 graphs, ', '| (b) trajectory, ONE launch, 3 frames x 3 graphs, ']),
    'bench_mol_scaffold': (TOY, ['| case | `pg_mol_rings` kernel ms, median (min - max) | `pg_mol_scaffold` kernel ms | scaffold / rings |'] + AB
                           + ['| (c) worst case: 3 graphs of 128 atoms, random logits (dense) |']),
    'bench_mol_props': (TOY, ['| case | `pg_mol_props` kernel ms, median (min - max) | `pg_mol_scaffold` kernel ms | props / scaffold |'] + AB
                        + ['| (c) 3 chains of 128 atoms, N or O in every fourth place |']),
    'bench_mol_sub': (TOY + ['--repeats', '2'], ['## (a) the sampler\'s final prediction, noise weights', '## (b) molecule-like graphs',
                                                 '| patterns | kernel ms, median (min - max) | us per (graph, pattern) |'] + SUB_ROWS),
    'bench_fingerprints': (TOY + ['--rows', '192', '--job_rows', '320', '--picks', '4'],
                           ['| frames | `pg_mol_fp` ms | `pg_mol_key` ms |', '| 1 | ', '| 3 | ', '| call | ms | T pairs/s | of the bound | torch ms |',
                            '| `pg_fp_tanimoto` 192 x 192 |', '| `pg_fp_nearest` 192 x 192 (self) |', '| `pg_fp_nearest` 320 x 320 (self) |',
                            '| `pg_fp_maxmin` 4 of 320 |']),
    # the two shape tools take no --graphs / --steps: their sets are synthetic, and their text is one JSON line per case
    'bench_shape': (['--sizes', '48', '--repeats', '2'], ['{"function": "similarity", "n_a": 48, "n_b": 48, ', '{"function": "nearest", "n_a": 48, "n_b": 48, ']),
    'bench_shape_align': (['--repeats', '1'], ['{"case": "1000 x 1 reference", "pairs": 1000, ', '{"case": "256 x 256", "pairs": 65536, ']),
}


def _timings(record):
    """Every number of a record (a dict, or a list of them) that is a time in ms, by its key."""
    if isinstance(record, list):
        return [t for r in record for t in _timings(r)]
    return [t for k, v in record.items() if 'ms' in k.split('_') or k.endswith(' ms') for t in (v if isinstance(v, list) else [v])]


def _keys(record):
    return [sorted(r) for r in record] if isinstance(record, list) else sorted(record)


@pytest.mark.parametrize('tool', sorted(CASES))
def test_tool_runs_at_toy_size(tool):
    argv, expected = CASES[tool]
    main = importlib.import_module(tool).main
    text, record = main(argv)
    lines = text.split('\n')
    for want in expected:
        n = sum(ln.startswith(want) for ln in lines)
        assert n == (2 if tool == 'bench_mol_sub' and want.startswith('|') else 1), (want, n, text)      # bench_mol_sub prints two tables
    times = _timings(record)
    assert times and all(isinstance(t, float) and math.isfinite(t) and t > 0 for t in times), record
    assert _keys(main(argv)[1]) == _keys(record)
