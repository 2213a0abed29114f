"""-m gpu: the SMILES kernel (csrc/mol_smiles.hip through phoregen_amd/molecule.py) against the plain restatement of
tests/smiles_reference.py, and the functions that carry its texts.  Integer work only: every comparison is `==`.  The restatement is
always fed the device's own kekule_order / hcount / charge, so the kernel's free choice of Kekulé structure does not enter; every
text is also read back by the independent reader to exactly the molecule the device holds."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kekule_reference as K
import mol_reference as R
import ring_reference as G
import smiles_reference as S
from helpers import default_model
from mol_support import split_frame, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CI = M.SMILES_COUNTS.index


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


@pytest.fixture(scope='module')
def family():
    """The random family of kekule_reference: built once, read by several tests, changed by none."""
    return K.random_family()


def _split(sm, sizes, f=0):
    """Frame f of a `Smiles` as one dict of host values per graph, in the restatement's form, plus the rows it was written from."""
    kk = sm.kekule
    out = split_frame(sizes, f, per_atom={'atom_rank': sm.atom_rank, 'cls': sm.screen.cls, 'hcount': kk.hcount, 'charge': kk.charge},
                      per_pair={'kekule_order': kk.kekule_order},
                      per_graph={'text': sm.text, 'length': sm.length, 'counts': sm.counts, 'status': sm.status, 'ok': sm.ok, 'kekule_status': kk.status})
    for r, string in zip(out, sm.strings(f)):
        row, n = r['text'], r['length']
        assert row.shape == (sm.capacity,) and not row[n:].any() and (row[:n] > 0x20).all() and (row[:n] < 0x7f).all()
        assert string == row[:n].tobytes().decode('ascii')
        r.update(text=string, rows=tuple(r.pop(k) for k in ('cls', 'kekule_order', 'hcount', 'charge', 'kekule_status')))
    return out


def _run(node, pos, edge, sizes, capacity=None, **kw):
    sm = M.smiles(_result(node, pos, edge, sizes), capacity=capacity, **kw)
    torch.cuda.synchronize()
    cap = capacity if capacity is not None else 8 * max(max(sizes, default=0), 8)
    assert sm.capacity == cap and sm.text.shape == (1, len(sizes), cap) and sm.status.shape == sm.ok.shape == sm.length.shape == (1, len(sizes))
    assert sm.counts.shape == (1, len(sizes), 8) and sm.atom_rank.shape == (1, sum(sizes))
    assert (sm.text.dtype, sm.length.dtype, sm.atom_rank.dtype, sm.counts.dtype, sm.status.dtype, sm.ok.dtype) == (
        torch.uint8, torch.int32, torch.int16, torch.int32, torch.int32, torch.bool)
    return sm, _split(sm, sizes)


def _validate(r, capacity=None, where=''):
    """One graph of the kernel: byte-equal to the restatement on the device's own Kekulé form, and read back exactly."""
    S.same_answer(r, S.smiles_of_rows(*r['rows'], capacity=capacity), where=where)
    assert r['ok'] == (r['status'] & M.SMILES_FAIL_MASK == 0)
    if r['ok']:
        S.check_read_back(r['text'], *r['rows'][:4], r['atom_rank'], where=where)


def _check(graphs, capacity=None, where=''):
    node, pos, edge, sizes = G.batch_from(graphs)
    sm, got = _run(node, pos, edge, sizes, capacity)
    for g, r in enumerate(got):
        _validate(r, capacity, where='%s %d' % (where, g))
    return sm, got


def test_examples_by_hand_twice_into_recycled_memory():
    graphs = [(c, b) for c, b, _ in S.EXAMPLES.values()]
    sm, got = _check(graphs, where='examples')
    assert [r['text'] for r in got] == [t for _, _, t in S.EXAMPLES.values()]
    by = dict(zip(S.EXAMPLES, got))
    assert by['tetrahedrane skeleton']['counts'].tolist() == [10, 4, 6, 1, 3, 0, 3, 0]
    assert by['tetramethylammonium']['counts'].tolist() == [14, 5, 4, 1, 0, 3, 0, 1] and by['tetramethylammonium']['status'] == M.SMILES_BRACKET
    assert by['dimethyl ether with a dropped atom']['atom_rank'].tolist() == [0, -1, 1, 2]
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    first = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != 'rows'} for r in got]
    del sm, got
    torch.empty(1 << 20, dtype=torch.uint8, device=DEV).fill_(0xEE)
    _, again = _check(graphs, where='again')
    for a, b in zip(first, again):
        assert all(np.array_equal(a[key], b[key]) for key in a)


def test_random_family(family):
    sm, got = _check(family, where='family')
    assert [len(c) for c, _ in family[:12]] == [1, 2, 3, 5, 6, 9, 10, 63, 64, 65, 127, 128]
    n_ok = sum(r['ok'] for r in got)
    n_none = sum(r['status'] == M.SMILES_NO_KEKULE for r in got)
    assert n_ok >= 14 and n_none >= 14 and n_ok + n_none == len(got)
    for r in got:
        c = dict(zip(M.SMILES_COUNTS, r['counts'].tolist()))
        if r['ok']:
            assert c['ring_closures'] == c['bonds'] - c['atoms'] + c['components'] and c['length'] == r['length'] == len(r['text'])
        else:
            assert r['text'] == '' and r['length'] == 0 and not r['counts'].any() and (r['atom_rank'] == -1).all()


def test_alone_and_inside_a_batch(family):
    pick = [g for g in range(len(family)) if len(family[g][0]) in (9, 10, 64, 65, 128)][:10]
    _, together = _check([family[g] for g in pick], where='together')
    for g, r in zip(pick, together):
        node, pos, edge, sizes = G.batch_from([family[g]])
        sm, (alone,) = _run(node, pos, edge, sizes, capacity=8 * 128)   # (the batch's row width: the same bytes and the same zeros)
        assert alone['text'] == r['text'] and alone['status'] == r['status'] and alone['length'] == r['length'], g
        assert np.array_equal(alone['counts'], r['counts']) and np.array_equal(alone['atom_rank'], r['atom_rank']), g
        assert all(np.array_equal(x, y) for x, y in zip(alone['rows'], r['rows'])), g


def test_renumbered_graphs(family):
    """Every text of a renumbered graph reads back exactly; atoms, bonds and components do not move, and ring_closures = bonds - atoms +
    components in both numberings.  The formula read back does not move either where the Kekulé structure is the neutral pass's: there
    the charges do not depend on the matching (only a four-valent N carries one), and `hydrogens - charge` never does (DESIGN.md 2.9
    "Kekulé form"), so neither do the hydrogens.  In the charged pass two maximum matchings may charge different numbers of atoms --
    the restatement alone, on this very batch, gives C53H107N4O4S2 3+ in one numbering and C53H106N4O4S2 2+ in the other for family
    graph 7 -- so there the elements and `hydrogens - charge` are held instead.  Which graphs are which is the Kekulé restatement's
    answer (the pass that decides is a property of the graph), not the kernel's."""
    graphs = list(family) + [(c, b) for c, b, _ in S.EXAMPLES.values()] + [K.NAMED[k][:2] for k in ('azulene', 'indole', 'N-methylpyridinium')]
    node, pos, edge, sizes = G.batch_from(graphs)
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=17)
    _, base = _run(node, pos, edge, sizes)
    _, moved = _run(node2, pos2, edge2, sizes)
    seen = charged = 0
    for g, (a, b) in enumerate(zip(base, moved)):
        _validate(b, where='renumbered %d' % g)
        assert a['ok'] == b['ok'] and (a['status'] & M.SMILES_FAIL_MASK) == (b['status'] & M.SMILES_FAIL_MASK), g
        if not a['ok']:
            continue
        for c in ('atoms', 'bonds', 'components'):
            assert a['counts'][CI(c)] == b['counts'][CI(c)], (g, c)
        for r in (a, b):
            assert r['counts'][CI('ring_closures')] == r['counts'][CI('bonds')] - r['counts'][CI('atoms')] + r['counts'][CI('components')], g
        if K.kekule_of_rows(*K.rows_of(*graphs[g]))['solution']['pass'] == 0:
            assert S.formula_of_text(a['text']) == S.formula_of_text(b['text']), (g, a['text'], b['text'])
            seen += 1
        else:
            (at_a, _), (at_b, _) = S.read_smiles(a['text']), S.read_smiles(b['text'])
            assert sorted(z for z, _, _ in at_a) == sorted(z for z, _, _ in at_b), g
            assert sum(h - q for _, h, q in at_a) == sum(h - q for _, h, q in at_b), g
            charged += 1
    assert seen >= 30 and charged >= 14


def test_label_and_capacity_boundaries():
    sm, (at, over) = _check([S.label_boundary(99), S.label_boundary(100)], where='labels')
    first = 'C' + ''.join(S.label_text(k) for k in range(1, 100))
    assert at['ok'] and at['text'].startswith(first + 'C') and first.endswith('%99') and at['counts'][CI('max_label')] == 99
    assert at['length'] <= sm.capacity == 1024
    assert (over['status'], over['text'], over['length'], over['counts'].tolist()) == (M.SMILES_RING_LABELS, '', 0, [0] * 8)
    assert (over['atom_rank'] == -1).all()
    classes, bonds = S.label_boundary(99)
    _, (one_more, later) = _check([(classes, {**bonds, (2, 127): 1}), (classes, {**bonds, (3, 127): 1})], where='closed here')
    assert one_more['status'] == M.SMILES_RING_LABELS and later['ok'] and later['counts'][CI('max_label')] == 99
    # capacity: the needed length passes, one byte fewer is TOO_LONG with the need in the count 'length'
    text = S.EXAMPLES['norbornane'][2]
    graphs = [S.EXAMPLES['norbornane'][:2], S.EXAMPLES['ethanol'][:2]]
    _, (exact, small) = _check(graphs, capacity=len(text), where='exact')
    assert exact['text'] == text and exact['status'] == 0 and small['text'] == 'CCO'
    _, (short, small) = _check(graphs, capacity=len(text) - 1, where='short')
    assert short['status'] == M.SMILES_TOO_LONG and short['text'] == '' and short['length'] == 0 and (short['atom_rank'] == -1).all()
    assert short['counts'].tolist() == exact['counts'].tolist() and short['counts'][CI('length')] == len(text) and small['text'] == 'CCO'
    _, (one, two) = _check(graphs, capacity=1, where='one byte')
    assert one['status'] == two['status'] == M.SMILES_TOO_LONG and two['counts'][CI('length')] == 3
    with pytest.raises(ValueError, match='capacity'):
        M.smiles(_result(*G.batch_from(graphs)[:3], [7, 3]), capacity=0)


def test_dropped_atom_absorbing_row_disconnected_and_empty():
    graphs = [([K.C_, K.C_, 11, K.C_, K.C_, K.C_], S.ring(6)),        # the ring opens: a chain of five, written from atom 0
              ([K.C_] * 6, {**S.ring(6), (2, 3): 5}),                 # a class-5 row in the ring: a chain of six
              ([K.N_] + [K.C_] * 5, {**K.cycle(6), (0, 3): 5, (1, 4): 5}),   # class-5 rows across an aromatic ring change nothing
              ([K.C_, K.O_, K.C_, K.C_, K.N_], {(0, 2): 1, (1, 3): 2}),   # three components
              ([11] * 5, S.ring(5))]                                  # nothing kept
    sm, got = _check(graphs, where='dropped')
    assert got[0]['text'] == 'C(C)CCC' and got[0]['atom_rank'].tolist() == [0, 1, -1, 4, 3, 2] and got[0]['status'] == 0
    assert got[1]['text'] == 'C(CC)CCC' and got[1]['counts'][CI('ring_closures')] == 0
    assert got[2]['ok'] and got[2]['counts'][CI('ring_closures')] == 1 and got[2]['text'].count('=') == 3 and got[2]['text'][0] == 'N'
    assert got[3]['text'] == 'CC.O=C.N' and got[3]['status'] == M.SMILES_DISCONNECTED and got[3]['counts'][CI('components')] == 3
    for r in got[4:]:
        assert (r['status'], r['text'], r['ok'], r['counts'].tolist()) == (M.SMILES_EMPTY, '', True, [0] * 8)
    assert int(sm.screen.status[0, 0]) & M.STATUS_HAD_MASKED_ATOM and int(sm.screen.status[0, 1]) & M.STATUS_HAD_ABSORBING_BOND
    assert int(sm.screen.status[0, 4]) & M.STATUS_NO_ATOMS


def test_trajectory_frames_and_reuse():
    """frames='traj', F = 3 in one launch: benzene / pyrrole, then one ring atom turned into O (no Kekulé structure), then a bond made
    single."""
    frames = [[([K.C_] * 6, K.cycle(6)), ([K.N_] + [K.C_] * 4, K.cycle(5))],
              [([K.O_] + [K.C_] * 5, K.cycle(6)), ([K.N_] + [K.C_] * 4, K.cycle(5))],
              [([K.C_] * 6, {**K.cycle(6), (0, 5): 1}), ([K.C_] * 5, K.cycle(5))]]
    per = [G.batch_from(f) for f in frames]
    sizes = per[0][3]
    traj = tuple(torch.stack([p[k] for p in per]).to(DEV) for k in range(3))
    res = _result(*per[-1][:3], sizes, traj=traj)
    sm = M.smiles(res, frames='traj')
    assert sm.status.shape == (3, 2) and sm.text.shape == (3, 2, 64) and sm.atom_rank.shape == (3, 11) and sm.kekule.status.shape == (3, 2)
    for f in range(3):
        for g, r in enumerate(_split(sm, sizes, f)):
            _validate(r, where='frame %d graph %d' % (f, g))
    N = M.SMILES_NO_KEKULE
    assert sm.status.tolist() == [[0, 0], [N, 0], [0, N]] and sm.ok.tolist() == [[True, True], [False, True], [True, False]]
    assert sm.strings(1) == ['', 'N1C=CC=C1'] and sm.strings(2)[1] == '' and sorted(sm.strings(0)[0]) == sorted('C1=CC=CC=C1')
    # a screen and a Kekulé form handed in are reused; ones of other frames, or of another result, are refused
    sc = M.screen(res, frames='traj')
    kk = M.kekulize(res, frames='traj', screen=sc)
    again = M.smiles(res, frames='traj', screen=sc, kekule=kk)
    assert again.screen is sc and again.kekule is kk and torch.equal(again.text, sm.text) and torch.equal(again.atom_rank, sm.atom_rank)
    assert M.smiles(res, frames='traj', kekule=kk).screen is sc
    with pytest.raises(ValueError, match='screen'):
        M.smiles(res, frames='final', kekule=kk)
    final = M.smiles(res)
    assert torch.equal(final.text[0], sm.text[2]) and torch.equal(final.status[0], sm.status[2])
    other = _result(*G.batch_from([([K.C_] * 6, K.cycle(6)), ([K.C_] * 5, S.ring(5))])[:3], [6, 5])
    assert M.smiles(res, kekule=M.kekulize(other)).strings()[1] == 'C1CCCC1'   # (equal sizes: taken as a screen of this result)
    with pytest.raises(ValueError, match='screen'):
        M.smiles(res, kekule=M.kekulize(_result(*G.batch_from([K.NAMED['benzene'][:2]])[:3], [6])))
    with pytest.raises(ValueError, match='different results'):
        M.smiles(res, screen=M.screen(res), kekule=M.kekulize(_result(*G.batch_from([([K.C_] * 5, S.ring(5)), ([K.C_] * 6, K.cycle(6))])[:3], [5, 6])))


def test_cpu_result_and_oversize_graph_are_refused():
    from phoregen_amd import hip
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.smiles({'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]})
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2

    class Rows:
        cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
        order = kekule_order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
        hcount = torch.zeros(1, n, dtype=torch.uint8, device=DEV)
        charge = torch.zeros(1, n, dtype=torch.int8, device=DEV)
        status = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
        lig_off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        bond_off = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    out = dict(status=torch.full((1, 1), 77, dtype=torch.int32, device=DEV), counts=torch.full((1, 1, 8), 77, dtype=torch.int32, device=DEV),
               text=torch.full((1, 1, 64), 77, dtype=torch.uint8, device=DEV), length=torch.full((1, 1), 77, dtype=torch.int32, device=DEV),
               atom_rank=torch.full((1, n), 77, dtype=torch.int16, device=DEV))
    table = M._smiles_table(Rows.cls.device)
    with pytest.raises(RuntimeError) as err:
        M._launch_smiles(hip.lib(), Rows, Rows, 1, 1, n, table, 64, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_smiles' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_smiles'):
        M._launch_smiles(hip.lib(), Rows, Rows, 1, 1, -1, table, 64, out)
    with pytest.raises(ValueError, match='smiles'):
        M._launch_smiles(hip.lib(), Rows, Rows, 1, 1, n, table[:10], 64, out)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())
    # empty batches return without a launch
    empty = M.smiles(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), []))
    assert empty.status.shape == (1, 0) and empty.text.shape == (1, 0, 64) and empty.strings() == []


def test_assemble_carries_the_smiles(tmp_path):
    names = ['N-methylpyridinium', 'indole', 'all-carbon five-ring', '2-pyridone']
    graphs = [K.NAMED[k][:2] for k in names] + [([K.C_, 11, K.C_, K.N_, K.C_, K.C_, K.C_, K.O_], {**K.cycle(5, off=2), (0, 2): 1, (4, 7): 1, (1, 2): 1})]
    node, pos, edge, sizes = G.batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    sm = M.smiles(res)
    got = _split(sm, sizes)
    plain, full = M.assemble(res), M.assemble(res, smiles=sm)
    for g, (p, m, r) in enumerate(zip(plain, full, got)):
        assert set(m) == set(p) | {'smiles'}
        for name in p:                                                 # the default output, key for key
            assert torch.equal(p[name], m[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], m[name]), name
        s = m['smiles']
        assert set(s) == {'status', 'smiles_ok', 'text', 'atom_rank'} | set(M.SMILES_COUNTS)
        assert [s[c] for c in M.SMILES_COUNTS] == r['counts'].tolist() and s['status'] == r['status'] and s['smiles_ok'] == r['ok']
        assert s['text'] == r['text'] and isinstance(s['text'], str)
        keep = r['rows'][0] >= 0
        assert s['atom_rank'].dtype == np.int16 and s['atom_rank'].tolist() == r['atom_rank'][keep].tolist() and len(s['atom_rank']) == len(m['element'])
    assert [m['smiles']['smiles_ok'] for m in full] == [True, True, False, True, True] and full[2]['smiles']['text'] == ''
    assert full[0]['smiles']['text'].startswith('[N+]') and full[0]['smiles']['status'] == M.SMILES_BRACKET
    # all five arguments ride in one copy, all from one screen; the text reads back to the dict's own atoms and Kekulé bonds
    pts, kinds = torch.tensor([[0.0, 0.0, 0.0], [4.0, 1.0, 0.0]]), torch.tensor([0, 3])
    geo = M.geometry(res, pts, torch.tensor([0, 1]), screen=sm.screen)
    rg = M.rings(res, screen=sm.screen)
    ft = M.features(res, pts, kinds, screen=sm.screen, kekule=sm.kekule, rings=rg)
    every = M.assemble(res, keys=True, geometry=geo, rings=rg, kekule=sm.kekule, features=ft, smiles=sm)
    without = M.assemble(res, keys=True, geometry=geo, rings=rg, kekule=sm.kekule, features=ft)
    for m, q, w in zip(every, without, full):
        assert set(m) == set(q) | {'smiles'} and m['key'] == q['key'] and m['geom']['status'] == q['geom']['status']
        assert m['rings']['status'] == q['rings']['status'] and m['features']['status'] == q['features']['status']
        assert m['kekule']['formula'] == q['kekule']['formula'] and torch.equal(m['kekule']['bond_type'], q['kekule']['bond_type'])
        assert all(np.array_equal(m['smiles'][k], w['smiles'][k]) for k in w['smiles'])
        if m['smiles']['smiles_ok']:
            atoms, bonds = S.read_smiles(m['smiles']['text'])
            rank = m['smiles']['atom_rank'].tolist()
            assert atoms == [(m['element'][i], int(m['kekule']['hcount'][i]), int(m['kekule']['charge'][i])) for i in np.argsort(rank)]
            want = {(min(rank[a], rank[b]), max(rank[a], rank[b])): t for (a, b), t in zip(m['bond_index'].T.tolist(), m['kekule']['bond_type'].tolist())}
            assert bonds == want and S.formula_of_text(m['smiles']['text']) == m['kekule']['formula']
    path = tmp_path / 's.sdf'
    M.write_sdf(str(path), every)
    text = path.read_text()
    assert text.count('> <PHOREGEN_SMILES>') == 4 and '> <PHOREGEN_SMILES>\n%s\n\n$$$$\n' % every[0]['smiles']['text'] in text
    with pytest.raises(ValueError, match='smiles='):                    # of another result
        M.assemble(res, smiles=M.smiles(_result(*G.batch_from([K.NAMED['benzene'][:2]])[:3], [6])))
    with pytest.raises(ValueError, match='smiles='):                    # of more than the final frame
        M.assemble(res, smiles=dataclasses.replace(sm, status=sm.status.repeat(2, 1)))
    swapped = _result(node, pos, edge, sizes[:3] + sizes[:2:-1])       # as many atom and bond rows, other graphs
    with pytest.raises(ValueError, match='different results'):
        M.assemble(res, rings=M.rings(swapped), smiles=sm)


def test_sample_valid_with_smiles(model):
    """Deterministic noise weights: what they decode to is unknown; whatever is finished has a text that reads back to its own atoms
    and Kekulé bonds, and finished and failed account for every draw."""
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    torch.manual_seed(5)
    drawn = []
    sample = model.sample

    class Counting:
        ex_col = getattr(model, 'ex_col', 12)

        def sample(self, data, n, device, **kw):
            drawn.append(n)
            return sample(data, n, device, **kw)
    out = M.sample_valid(Counting(), data, num_samples=4, batch_size=4, max_failed_factor=1, smiles=True, kekule=True, num_steps=10)
    assert set(out) == {'finished', 'failed', 'n_calls'} and out['n_calls'] == len(drawn) >= 1
    assert len(out['finished']) + len(out['failed']) == sum(drawn)
    assert len(out['finished']) == 4 or len(out['failed']) > 4
    for m in out['finished']:
        assert m['valid'] and m['smiles']['smiles_ok'] and m['kekule']['kekule_ok']
        atoms, bonds = S.read_smiles(m['smiles']['text'])
        rank = m['smiles']['atom_rank'].tolist()
        assert [z for z, _, _ in atoms] == [m['element'][i] for i in np.argsort(rank)]
        assert bonds == {(min(rank[a], rank[b]), max(rank[a], rank[b])): t
                         for (a, b), t in zip(m['bond_index'].T.tolist(), m['kekule']['bond_type'].tolist())}
    for m in out['failed']:
        assert not m['valid'] or not m['smiles']['smiles_ok']
    # a stand-in model that hands out pyridine, the all-carbon five-ring and thiopyrylium in turn
    parts = [R.scores_from_classes(*K.NAMED[k][:2]) for k in ('pyridine', 'all-carbon five-ring', 'thiopyrylium')]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % 3] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [p[0].size(0) for p in pick])
    out = M.sample_valid(Rota(), None, num_samples=4, batch_size=3, smiles=True)
    assert all('kekule' not in m and m['smiles']['smiles_ok'] for m in out['finished']) and len(out['finished']) == 4   # 'kekule' only if asked for
    assert sorted({S.formula_of_text(m['smiles']['text']) for m in out['finished']}) == ['C5H5N', 'C5H5S+']
    assert all(m['smiles']['status'] == M.SMILES_NO_KEKULE for m in out['failed']) and len(out['failed']) >= 1
    out = M.sample_valid(Rota(), None, num_samples=2, batch_size=3, smiles=True, kekule=M.KekuleOptions(allow_charged=False), max_failed_factor=2)
    assert [m['kekule']['formula'] for m in out['finished']] == ['C5H5N', 'C5H5N'] == [S.formula_of_text(m['smiles']['text']) for m in out['finished']]


def test_sample_cli_writes_the_smiles_file(tmp_path):
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    out = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(out), '--smiles', '--sdf', '--num_steps', '10'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(out.glob('*.pt'))), weights_only=False)
    (path,) = out.glob('*_SMILES_all.txt')
    lines = path.read_text().split('\n')
    assert lines[-1] == '' and lines[:-1] == [m['smiles']['text'] for m in done] and all(m['smiles']['smiles_ok'] for m in done)
    for ln in lines[:-1]:
        S.read_smiles(ln)
    sdfs = sorted((out / 'sdf_results').glob('*.sdf'))
    assert len(sdfs) == len(done) and all('> <PHOREGEN_SMILES>' in p.read_text() for p in sdfs)
