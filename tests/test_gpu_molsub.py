"""-m gpu: the substructure kernel (csrc/mol_sub.hip through phoregen_amd/substructure.py) against the plain restatement of
tests/sub_reference.py.  Integer work: every comparison is `==`.  The restatement is handed the ring and Kekulé outputs of the device
(each held against its own restatement in tests/test_gpu_molrings.py / test_gpu_molkekule.py): which Kekulé structure `kekulize`
returns is not canonical, so the hydrogens of an aromatic atom are an input here, not something to restate."""
import os

import numpy as np
import pytest
import torch

import mol_reference as MR
import molkey_reference as Q
import ring_reference as G
import sub_reference as R
from helpers import default_model
from mol_support import M64, split_frame, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import substructure as S
from phoregen_amd.utils.sample_utils import ATOM_TYPES

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICTS = R.PATTERNS + R.PROPERTY_PATTERNS
PATTERNS = [S.Pattern.from_dict(p) for p in DICTS]


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _targets(sc, rg, kek, f=0):
    """The restatement's targets of frame f from the device's screen, ring and Kekulé outputs."""
    parts = split_frame(sc.num_atoms, f, per_atom={'cls': sc.cls, 'atom_ring': rg.atom_ring, 'hcount': kek.hcount, 'charge': kek.charge},
                        per_pair={'order': sc.order, 'ring_size': rg.ring_size}, per_graph={'kekule_status': kek.status})
    return [R.target_of_rows(**r) for r in parts]


def _rows(sub, f=0):
    """[graph][pattern] -> the row dict of sub_reference.check_row, from one device-to-host copy per tensor"""
    emb, anc, status = sub.embeddings[f].cpu().tolist(), sub.anchors[f].cpu().tolist(), sub.status[f].cpu().tolist()
    mask, first = sub.atom_mask[f].cpu().tolist(), sub.first[f].cpu().tolist()
    return [[{'embeddings': emb[g][p], 'anchors': anc[g][p], 'mask': (mask[g][p][0] & M64) | (mask[g][p][1] & M64) << 64,
              'first': first[g][p], 'status': status[g][p]} for p in range(len(sub.patterns))] for g in range(len(emb))]


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ('embeddings', 'anchors', 'atom_mask', 'first', 'status', 'ok'))


@pytest.fixture(scope='module')
def ragged():
    """The ragged batch, its device outputs and the restatement's rows [graph][pattern], computed once."""
    node, pos, edge, sizes = MR.generate_batch()
    res = _result(node, pos, edge, sizes)
    sc = M.screen(res)
    rg, kek = M.rings(res, screen=sc), M.kekulize(res, screen=sc)
    targets = _targets(sc, rg, kek)
    want = [[R.search(t, p) for p in DICTS] for t in targets]
    return dict(node=node, pos=pos, edge=edge, sizes=sizes, res=res, sc=sc, rg=rg, kek=kek, targets=targets, want=want)


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement_on_the_ragged_batch(ragged):
    sizes, want, targets = ragged['sizes'], ragged['want'], ragged['targets']
    for n in (1, 2, 3, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    assert len(sizes) == 160 and len(PATTERNS) == 20
    # on the restatement alone, before the kernel is looked at
    assert not any(w['truncated'] for row in want for w in row)
    assert any(len(t['atoms']) > 64 and w['mask'] & M64 and w['mask'] >> 64 for t, row in zip(targets, want) for w in row)
    assert sum(not t['atoms'] for t in targets) >= 2 and sum(len(t['atoms']) < n for t, n in zip(targets, sizes)) >= 10
    assert sum(t['kekule_failed'] for t in targets) >= 1 and sum(w['no_kekule'] for row in want for w in row) >= 4
    for i, p in enumerate(DICTS):
        assert any(row[i]['embeddings'] for row in want) or p['name'] in ('aromatic-ring', 'fused-bicycle'), p['name']
    sub = S.substructure(ragged['res'], PATTERNS, screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek'])
    torch.cuda.synchronize()
    B, P = len(sizes), len(PATTERNS)
    assert sub.embeddings.shape == sub.anchors.shape == sub.status.shape == (1, B, P) and sub.embeddings.dtype == torch.int32
    assert sub.atom_mask.shape == (1, B, P, 2) and sub.atom_mask.dtype == torch.int64
    assert sub.first.shape == (1, B, P, S.MAX_ATOMS) and sub.first.dtype == torch.int16 and sub.ok.shape == (1, B) and sub.ok.dtype == torch.bool
    got = _rows(sub)
    for g in range(B):
        for i, p in enumerate(DICTS):
            R.check_row(got[g][i], want[g][i], targets[g], p, (g, sizes[g], p['name']))
    assert sub.ok[0].tolist() == [not any(w['status'] & S.SUB_OUT_OF_BOUNDS for w in row) for row in want]
    assert 0 < int(sub.ok.sum()) < B
    # whichever of the screen, the rings and the Kekulé form is missing is computed
    assert _same(S.substructure(ragged['res'], PATTERNS), sub)
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    shapes = {k: getattr(sub, k).shape for k in ('embeddings', 'anchors', 'atom_mask', 'first', 'status')}
    keep = sub
    del sub
    for _ in range(2):
        junk = [torch.full(tuple(s), -1, dtype=getattr(keep, k).dtype, device=DEV) for k, s in shapes.items()]
        del junk
        assert _same(S.substructure(ragged['res'], PATTERNS, screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek']), keep)


def test_a_graph_alone_and_a_pattern_alone(ragged):
    sizes = ragged['sizes']
    sub = S.substructure(ragged['res'], PATTERNS, screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek'])
    n_off = np.concatenate([[0], np.cumsum(sizes)])
    e_off = np.concatenate([[0], np.cumsum([n * (n - 1) for n in sizes])])
    for g in (0, 3, 5, 8, 9, 20, 47):                                  # sizes 1, 16, 63, 78, 128, an all-masked graph, a small one
        one = _result(ragged['node'][n_off[g]:n_off[g + 1]], ragged['pos'][n_off[g]:n_off[g + 1]], ragged['edge'][e_off[g]:e_off[g + 1]],
                      [sizes[g]])
        alone = S.substructure(one, PATTERNS)
        for k in ('embeddings', 'anchors', 'atom_mask', 'first', 'status'):
            assert torch.equal(getattr(alone, k)[0, 0], getattr(sub, k)[0, g]), (g, k)
    for i in (0, 5, 11, 12, 16, 19):
        alone = S.substructure(ragged['res'], [PATTERNS[i]], screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek'])
        for k in ('embeddings', 'anchors', 'atom_mask', 'first', 'status'):
            assert torch.equal(getattr(alone, k)[:, :, 0], getattr(sub, k)[:, :, i]), (i, k)
    # and the order of the patterns in the table does not matter
    back = S.substructure(ragged['res'], PATTERNS[::-1], screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek'])
    assert torch.equal(back.embeddings.flip(-1), sub.embeddings) and torch.equal(back.first.flip(-2), sub.first)


def test_renumbered_batch_has_the_same_counts(ragged):
    node, pos, edge, sizes = (ragged[k] for k in ('node', 'pos', 'edge', 'sizes'))
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=5)
    assert not torch.equal(node, node2)
    # (patterns that read hydrogens or charge are left out: the Kekulé structure chosen may move a hydrogen with the numbering)
    idx = [i for i, p in enumerate(PATTERNS) if not p.uses_kekule]
    assert len(idx) == 16
    pats = [PATTERNS[i] for i in idx]
    a = S.substructure(ragged['res'], pats, screen=ragged['sc'], rings=ragged['rg'], kekule=ragged['kek'])
    res2 = _result(node2, pos2, edge2, sizes)
    b = S.substructure(res2, pats)
    assert torch.equal(a.embeddings, b.embeddings) and torch.equal(a.anchors, b.anchors) and torch.equal(a.status, b.status)
    assert int(a.embeddings.sum()) > 1000
    # the masks are permuted accordingly: local atom i became perms[g][i]; compare as sets of local atoms
    ca, cb = a.screen.compact[0].cpu().numpy(), b.screen.compact[0].cpu().numpy()
    ma, mb = _rows(a), _rows(b)
    n0 = 0
    for g, n in enumerate(sizes):
        local_a = {int(c): i for i, c in enumerate(ca[n0:n0 + n]) if c >= 0}
        local_b = {int(c): i for i, c in enumerate(cb[n0:n0 + n]) if c >= 0}
        for i in range(len(pats)):
            moved = {int(perms[g][local_a[c]]) for c in S.mask_atoms(R.mask_words(ma[g][i]['mask']))}
            assert moved == {local_b[c] for c in S.mask_atoms(R.mask_words(mb[g][i]['mask']))}, (g, i)
        n0 += n
    # and the permuted batch equals its own restatement, so the agreement is not two equal mistakes
    targets = _targets(b.screen, b.rings, b.kekule)
    for g in range(0, len(sizes), 7):
        for i, p in zip(range(len(pats)), (DICTS[j] for j in idx)):
            R.check_row(mb[g][i], R.search(targets[g], p), targets[g], p, (g, p['name']))


# ---- the work bound ------------------------------------------------------------------------------------------------------------------
def test_truncation_on_the_corpus():
    mols, _, _, names = Q.corpus()
    graphs = []
    for m in mols:
        bi, bt = m['bond_index'].numpy(), m['bond_type'].numpy()
        graphs.append(([ATOM_TYPES.index(z) for z in m['element']], {(int(a), int(b)): int(t) for a, b, t in zip(bi[0], bi[1], bt)}))
    node, pos, edge, sizes = G.batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    pats = PATTERNS[:len(R.PATTERNS)] + [S.Pattern.from_dict(dict(R.PATTERNS[7], name='6-cycle-required', min=1))]
    dicts = R.PATTERNS + [dict(R.PATTERNS[7], name='6-cycle-required', min=1)]
    sub = S.substructure(res, pats, max_steps=100)
    targets = _targets(sub.screen, sub.rings, sub.kekule)
    want = [[R.search(t, p, max_steps=100) for p in dicts] for t in targets]
    truncated = {p['name'] for row in want for p, w in zip(dicts, row) if w['truncated']}
    assert truncated == {'fused-bicycle', '6-cycle', '5-cycle', 'path-16', '6-cycle-required'}
    assert sum(w['truncated'] for row in want for w in row) >= 20
    got = _rows(sub)
    lower = 0
    for g, t in enumerate(targets):
        for i, p in enumerate(dicts):
            R.check_row(got[g][i], want[g][i], t, p, (names[g], p['name']))
            lower += want[g][i]['truncated'] and 0 < got[g][i]['embeddings'] < want[g][i]['embeddings']
    assert lower >= 1                                                  # a truncated row that found something, and not everything
    # at the default bound nothing truncates and every row is exact
    full = S.substructure(res, pats, screen=sub.screen, rings=sub.rings, kekule=sub.kekule)
    assert not bool((full.status & S.SUB_TRUNCATED).any())
    got = _rows(full)
    for g in range(0, len(targets), 5):
        for i, p in enumerate(dicts):
            R.check_row(got[g][i], R.search(targets[g], p), targets[g], p, (names[g], p['name']))


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def test_three_strided_frames_equal_three_calls():
    sizes = [5, 17, 66, 3, 30]
    rng = np.random.default_rng(3)
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    node = torch.from_numpy(rng.normal(0, 1, (6, N, 12)).astype(np.float32))
    node[..., 1] += 1.5                                                # mostly carbon
    edge = torch.from_numpy(rng.normal(0, 1, (6, E, 6)).astype(np.float32))
    edge[..., 0] += 4.0                                                # mostly "no bond", else the searches explode
    pos = torch.from_numpy(rng.normal(0, 3, (6, N, 3)).astype(np.float32))
    full = _result(node[-1], pos[-1], edge[-1], sizes, traj=(node.to(DEV), pos.to(DEV), edge.to(DEV)))
    strided = dict(full, traj=[t[::2] for t in full['traj']])
    assert not strided['traj'][0].is_contiguous()
    sub = S.substructure(strided, PATTERNS, frames='traj', max_steps=20000)
    assert sub.embeddings.shape == (3, len(sizes), len(PATTERNS)) and sub.ok.shape == (3, len(sizes))
    for f in range(3):
        one = S.substructure(_result(node[2 * f], pos[2 * f], edge[2 * f], sizes), PATTERNS, max_steps=20000)
        for k in ('embeddings', 'anchors', 'atom_mask', 'first', 'status', 'ok'):
            assert torch.equal(getattr(one, k)[0], getattr(sub, k)[f]), (f, k)
    assert int(sub.embeddings.sum()) > 0 and not torch.equal(sub.embeddings[0], sub.embeddings[1])
    targets = _targets(sub.screen, sub.rings, sub.kekule, f=1)
    got = _rows(sub, f=1)
    for g, t in enumerate(targets):
        for i, p in enumerate(DICTS):
            R.check_row(got[g][i], R.search(t, p, max_steps=20000), t, p, (g, p['name']))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    small = M.screen(_result(*MR.scores_from_classes([1, 1, 3], {(0, 1): 1, (1, 2): 1})[:3], [3]))
    res = _result(*MR.scores_from_classes([1, 1, 3], {(0, 1): 1, (1, 2): 1})[:3], [3])
    rg, kek = M.rings(res, screen=small), M.kekulize(res, screen=small)
    host = S.pattern_table(PATTERNS[:2])
    table = torch.from_numpy(host).to(DEV)
    big_host = np.tile(host[:1], (257, 1))
    big = torch.from_numpy(big_host).to(DEV)

    def outputs(P):
        return dict(embeddings=torch.full((1, 1, P), 77, dtype=torch.int32, device=DEV), anchors=torch.full((1, 1, P), 77, dtype=torch.int32, device=DEV),
                    atom_mask=torch.full((1, 1, P, 2), 77, dtype=torch.int64, device=DEV),
                    first=torch.full((1, 1, P, S.MAX_ATOMS), 77, dtype=torch.int16, device=DEV),
                    status=torch.full((1, 1, P), 77, dtype=torch.int32, device=DEV))

    def untouched(out):
        torch.cuda.synchronize()
        return all(bool((t == 77).all()) for t in out.values())

    lib = hip.lib()
    out = outputs(257)
    for P, message in ((0, '0 patterns'), (257, '257 patterns')):
        with pytest.raises(RuntimeError, match='pg_mol_sub: ' + message):
            S._launch_sub(lib, small, rg, kek, 1, 1, 3, big, big_host, P, 100, out)
    for steps in (0, -1):
        with pytest.raises(RuntimeError, match='pg_mol_sub: max_steps'):
            S._launch_sub(lib, small, rg, kek, 1, 1, 3, table, host, 2, steps, out)
    for off, value, message in ((hip.PG_SUB_OFF_K, 17, 'k outside 1'), (hip.PG_SUB_OFF_K, 0, 'k outside 1'),
                                (hip.PG_SUB_OFF_ATOMS, 0, 'empty element set'), (hip.PG_SUB_OFF_BONDS + 1, 16, 'empty order set'),
                                (hip.PG_SUB_OFF_BONDS + 1, 0, 'without a bond to an earlier one')):
        bad = host.copy()
        bad[1, off] = value
        if off == hip.PG_SUB_OFF_ATOMS:
            bad[1, off + 1] = 0
        if off == hip.PG_SUB_OFF_BONDS + 1 and value == 0:
            bad[1, hip.PG_SUB_OFF_BONDS + 16] = 0
        with pytest.raises(RuntimeError, match='pattern 1 is malformed.*' + message):
            S._launch_sub(lib, small, rg, kek, 1, 1, 3, torch.from_numpy(bad).to(DEV), bad, 2, 100, out)
    with pytest.raises(RuntimeError, match='pg_mol_sub: B 1, F 1'):
        S._launch_sub(lib, small, rg, kek, 1, 1, -1, table, host, 2, 100, out)
    assert untouched(out)
    # a graph of 129 atoms
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    from types import SimpleNamespace as NS
    sc_big = NS(cls=torch.zeros(1, n, dtype=torch.int8, device=DEV), order=torch.zeros(1, h, dtype=torch.int8, device=DEV),
                compact=torch.zeros(1, n, dtype=torch.int16, device=DEV), lig_off=torch.tensor([0, n], dtype=torch.int32, device=DEV),
                bond_off=torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV))
    rg_big = NS(ring_size=torch.zeros(1, h, dtype=torch.uint8, device=DEV), atom_ring=torch.zeros(1, n, dtype=torch.uint8, device=DEV))
    kek_big = NS(hcount=torch.zeros(1, n, dtype=torch.uint8, device=DEV), charge=torch.zeros(1, n, dtype=torch.int8, device=DEV),
                 status=torch.zeros(1, 1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError) as err:
        S._launch_sub(lib, sc_big, rg_big, kek_big, 1, 1, n, table, host, 2, 100, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and str(n) in str(err.value) and untouched(out)
    # the Python surface refuses its own share with a ValueError
    for bad_steps in (0, 2 ** 30 + 1, 1.5, True):
        with pytest.raises(ValueError, match='max_steps'):
            S.substructure(res, PATTERNS[:2], max_steps=bad_steps)
    with pytest.raises(ValueError, match='Pattern objects'):
        S.substructure(res, [])
    other = M.screen(_result(*MR.scores_from_classes([1, 1], {(0, 1): 1})[:3], [2]))
    with pytest.raises(ValueError, match='not one of this result|different results'):
        S.substructure(res, PATTERNS[:2], screen=other)
    # and the good call writes every element: C-C-O has one C-O bond, no C=any
    good = outputs(2)
    S._launch_sub(lib, small, rg, kek, 1, 1, 3, table, host, 2, 100, good)
    torch.cuda.synchronize()
    assert good['embeddings'].reshape(-1).tolist() == [3, 1] and good['anchors'].reshape(-1).tolist() == [3, 1]
    assert good['atom_mask'].reshape(-1).tolist() == [7, 0, 6, 0] and good['status'].reshape(-1).tolist() == [1, 1]
    assert good['first'].reshape(2, -1).tolist() == [[0] + [-1] * 15, [1, 2] + [-1] * 14]
    # empty batches return without a launch
    empty = S.substructure(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), []), PATTERNS[:2])
    assert empty.embeddings.shape == (1, 0, 2) and empty.ok.shape == (1, 0)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
REQUIRED = {'name': 'C-C', 'atoms': [{'elements': ['C']}, {'elements': ['C']}], 'bonds': [{'a': 0, 'b': 1}], 'min': 1}
FORBIDDEN = {'name': 'crowded-atom', 'atoms': [{'degree': [4, 255]}], 'max': 0}


def _within(mol, pattern):
    anchors = len({e[0] for e in S.find_matches(mol, pattern)})
    return anchors >= pattern.min and (pattern.max is None or anchors <= pattern.max)


def test_sample_valid_assemble_and_sdf_end_to_end(model, tmp_path):
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    pats = [S.Pattern.from_dict(REQUIRED), S.Pattern.from_dict(FORBIDDEN)]
    torch.manual_seed(5)
    out = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=1, num_steps=10, substructure=pats)
    assert out['n_calls'] >= 1 and len(out['finished']) + len(out['failed']) >= 4
    for m in out['finished']:
        assert m['valid'] and m['substructure_ok'] and all(_within(m, p) for p in pats)
    for m in out['failed']:
        assert not m['valid'] or (not m['substructure_ok'] and not all(_within(m, p) for p in pats))
    # assemble(substructure=) carries the tensors' values, and leaves every other key as it was
    from bench import ligphore_workload
    NA = [11, 9, 14, 8]
    w = ligphore_workload(len(NA), seed=11)
    centers = torch.randn(len(NA), 3, generator=torch.Generator().manual_seed(11)) * 2.0
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(NA), centers, rng='device',
                             seed=17, num_steps=10)
    torch.cuda.synchronize()
    # (ten steps of noise weights leave dense graphs: patterns of at most four atoms, so that no search is cut short)
    sub = S.substructure(res, [q for q in PATTERNS if q.k <= 4] + pats)
    assert len(sub.patterns) == 16 and not bool((sub.status & S.SUB_TRUNCATED).any())
    plain = M.assemble(res)
    mols = M.assemble(res, substructure=sub, rings=sub.rings, kekule=sub.kekule)
    rows = _rows(sub)
    for g, (p, m) in enumerate(zip(plain, mols)):
        assert set(m) == set(p) | {'substructure', 'substructure_ok', 'rings', 'kekule'}
        for name in p:
            same = torch.equal(p[name], m[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], m[name])
            assert same, name
        assert list(m['substructure']) == [q.name for q in sub.patterns] and m['substructure_ok'] == bool(sub.ok[0, g])
        for i, q in enumerate(sub.patterns):
            e, r = m['substructure'][q.name], rows[g][i]
            assert (e['embeddings'], e['anchors'], e['status']) == (r['embeddings'], r['anchors'], r['status'])
            assert e['atoms'] == S.mask_atoms(R.mask_words(r['mask'])) and e['status_names'] == S.status_names(r['status'])
            assert e['first'] == (r['first'][:q.k] if r['embeddings'] else None)
            found = S.find_matches(m, q)                               # the host enumerator on the assembled molecule agrees
            assert len(found) == e['embeddings'] and (list(found[0]) if found else None) == e['first']
    only = M.assemble(res, substructure=sub)
    assert [m['substructure'] for m in only] == [m['substructure'] for m in mols] and 'rings' not in only[0]
    # write_sdf round-trips the data item
    path = tmp_path / 'mols.sdf'
    M.write_sdf(str(path), mols)
    records = path.read_text().split('$$$$\n')[:-1]
    assert len(records) == len(mols)
    for text, m in zip(records, mols):
        assert S.parse_sdf_item(text) == m['substructure']
    M.write_sdf(str(path), plain)
    assert 'PHOREGEN_SUBSTRUCTURE' not in path.read_text()


def test_a_fixed_fragment_is_found_where_it_was_put(model):
    from bench import ligphore_workload
    from phoregen_amd.fragment import Fragment
    frag = Fragment.from_dict({'element': [6, 7, 8], 'pos': [[0.0, 0.0, 0.0], [1.4, 0.0, 0.0], [-0.7, 1.2, 0.0]], 'bonds': [(0, 1, 1), (0, 2, 2)]})
    NA = [9, 6, 12]
    w = ligphore_workload(len(NA), seed=7)
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(NA), torch.zeros(len(NA), 3),
                             rng='device', seed=3, num_steps=10, fragments=[frag] * len(NA))
    torch.cuda.synchronize()
    pattern = S.Pattern.from_fragment(frag, name='kept-fragment', min=1)
    sub = S.substructure(res, [pattern])
    compact = sub.screen.compact[0].cpu().tolist()
    n0 = 0
    for g, n in enumerate(NA):
        assert compact[n0:n0 + 3] == [0, 1, 2]                         # the fragment's atoms are the graph's first, and kept
        assert int(sub.embeddings[0, g, 0]) >= 1 and bool(sub.ok[0, g])
        assert sub.first[0, g, 0, :3].tolist() == [0, 1, 2] and int(sub.atom_mask[0, g, 0, 0]) & 7 == 7
        n0 += n
    mols = M.assemble(res, substructure=sub)
    assert all((0, 1, 2) in S.find_matches(m, pattern) for m in mols)
