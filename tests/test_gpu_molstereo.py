"""-m gpu: the stereo kernel (csrc/mol_stereo.hip) and the isomeric SMILES (pg_mol_smiles_stereo in csrc/mol_smiles.hip) through
phoregen_amd/molecule.py against the plain restatement of tests/stereo_reference.py, and the functions that carry their answers.
The restatement is always fed the device's own screen, Kekulé form, rings and colours, so only the kernels under test enter.
Perception is integer work but for two fp32 values compared with a threshold; the generated family keeps every such value 1e-4 away
from it (asserted on the restatement in tests/test_molstereo_host.py), so every comparison is `==`.  Every text is also read back
by the independent reader and held against the coordinates in float64."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kekule_reference as K
import smiles_reference as S
import stereo_reference as T
from mol_support import M64, MolRows, split_frame, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def family():
    """The generated family: built once, read by several tests, changed by none."""
    return T.family()


def _split(st, sm, pos, sizes, f=0):
    """Frame f of a `Stereo` and of the `Smiles` written with it as one dict of host values per graph: 'stereo' and 'text' in the
    restatement's forms, 'rows' = the `all_rows` record of the device's own inputs."""
    sc, kk = st.screen, st.kekule
    stereo = split_frame(sizes, f, per_atom={'atom_parity': st.atom_parity, 'atom_label': st.atom_label},
                         per_pair={'bond_stereo': st.bond_stereo, 'bond_label': st.bond_label},
                         per_graph={'stereo_key': st.stereo_key, 'counts': st.counts, 'status': st.status})
    texts = split_frame(sizes, f, per_atom={'atom_rank': sm.atom_rank},
                        per_graph={'bytes': sm.text, 'status': sm.status, 'length': sm.length, 'counts': sm.counts, 'stereo_counts': sm.stereo_counts})
    rows = split_frame(sizes, f, per_atom={'cls': sc.cls, 'hcount': kk.hcount, 'charge': kk.charge, 'colour': st.keys.colour},
                       per_pair={'order': sc.order, 'kekule_order': kk.kekule_order, 'ring_size': st.rings.ring_size},
                       per_graph={'kekule_status': kk.status, 'key': st.keys.key})
    out = []
    for s, t, m, p, string in zip(stereo, texts, rows, np.split(np.asarray(pos, dtype=np.float64), np.cumsum(sizes, dtype=int)[:-1]), sm.strings(f)):
        row = t.pop('bytes')
        assert not row[t['length']:].any() and string == row[:t['length']].tobytes().decode('ascii')
        s['stereo_key'] &= M64
        m.update(colour=[int(c) & M64 for c in m['colour']], key=m['key'] & M64)
        out.append({'stereo': s, 'text': dict(t, text=string, ok=t['status'] & M.SMILES_FAIL_MASK == 0), 'rows': MolRows(pos=p, **m)})
    return out


def _run(graphs, limits=M.StereoLimits(), capacity=None):
    node, pos, edge, sizes = T.batch_from(graphs)
    res = _result(node, pos, edge, sizes)
    st = M.stereo(res, limits=limits)
    sm = M.smiles(res, stereo=st, capacity=capacity)
    torch.cuda.synchronize()
    B, N, H = len(sizes), sum(sizes), sum(n * (n - 1) // 2 for n in sizes)
    assert st.status.shape == st.ok.shape == st.stereo_key.shape == (1, B) and st.counts.shape == (1, B, 8)
    assert st.atom_parity.shape == st.atom_label.shape == (1, N) and st.bond_stereo.shape == st.bond_label.shape == (1, H)
    assert (st.atom_parity.dtype, st.bond_label.dtype, st.stereo_key.dtype, st.counts.dtype, st.status.dtype) == (
        torch.int8, torch.int8, torch.int64, torch.int32, torch.int32)
    cap = capacity if capacity is not None else 12 * max(max(sizes, default=0), 8)
    assert sm.capacity == cap and sm.text.shape == (1, B, cap) and sm.stereo_counts.shape == (1, B, 4) and sm.stereo is st and sm.kekule is st.kekule
    return res, st, sm, _split(st, sm, pos.numpy(), sizes)


def _validate(r, limits=None, capacity=None, where=''):
    """One graph: every output `==` the restatement's on the device's own inputs; the text agrees with the coordinates."""
    rows = r['rows']
    want = T.restate(rows, limits)
    T.same_stereo(r['stereo'], want, where=where)
    T.same_text(r['text'], T.smiles_of_rows(*rows.smiles_inputs(), want['atom_parity'], want['bond_stereo'], capacity=capacity), where=where)
    if r['text']['ok']:
        _, _, at = T.graph_of_rows(rows.cls, rows.order)
        return T.check_text_against_geometry(r['text']['text'], r['text']['atom_rank'], rows.pos, want, at, limits, where=where)
    return 0, 0, 0


def _facts(r):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for part in ('stereo', 'text') for k, v in r[part].items()}


def test_examples_by_hand_their_mirror_images_twice_into_recycled_memory():
    graphs = T.example_graphs() + [(c, b, np.array(T.mirrored(p), dtype=np.float32)) for c, b, p, _ in T.EXAMPLES.values()]
    n = len(T.EXAMPLES)
    res, st, sm, got = _run(graphs)
    for g, r in enumerate(got):
        _validate(r, where='example %d' % g)
    by, mirror = dict(zip(T.EXAMPLES, got[:n])), dict(zip(T.EXAMPLES, got[n:]))
    assert [r['text']['text'] for r in got[:n]] == [t for _, _, _, t in T.EXAMPLES.values()]
    assert mirror['CHFClBr skeleton']['text']['text'] == '[C@@H](F)(Cl)Br' and mirror['cis-1,2-difluoroethene skeleton']['text']['text'] == 'F/C=C\\F'
    for name in ('ring double bond', 'allene'):
        assert not by[name]['stereo']['counts'].any() and by[name]['stereo']['stereo_key'] == by[name]['rows'].key
    assert by['conjugated triene']['stereo']['counts'].tolist() == [0, 0, 0, 0, 3, 3, 3, 0]
    assert by['quaternary N+']['text']['text'].startswith('[N@+]') and by['quaternary N+']['stereo']['status'] == M.STEREO_HAS_CENTRE
    assert by['oxime']['stereo']['status'] == M.STEREO_HAS_BOND and by['oxime']['text']['stereo_counts'].tolist() == [0, 0, 2, 1]
    # reflection: every atom label flips, bond labels and bond stereo stay; a chiral key moves, a meso one and one without centres stay
    for name in T.EXAMPLES:
        a, b = by[name]['stereo'], mirror[name]['stereo']
        assert b['atom_label'].tolist() == [-x if abs(x) == 1 else x for x in a['atom_label'].tolist()], name
        assert b['bond_label'].tolist() == a['bond_label'].tolist() and b['bond_stereo'].tolist() == a['bond_stereo'].tolist(), name
        chiral = name in ('CHFClBr skeleton', 'quaternary N+', 'chiral tartaric skeleton', 'centre that is a ring-closure atom')
        assert (a['stereo_key'] != b['stereo_key']) == chiral, name
    assert by['meso-tartaric skeleton']['stereo']['stereo_key'] != by['chiral tartaric skeleton']['stereo']['stereo_key']
    assert by['meso-tartaric skeleton']['rows'].key == by['chiral tartaric skeleton']['rows'].key
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    first = [_facts(r) for r in got]
    del res, st, sm, got
    torch.empty(1 << 21, dtype=torch.uint8, device=DEV).fill_(0xEE)
    _, _, _, again = _run(graphs)
    assert [_facts(r) for r in again] == first


def test_generated_family_and_plain_text_without_stereo(family):
    res, st, sm, got = _run(family)
    centres = doubles = 0
    for g, r in enumerate(got):
        a, b, _ = _validate(r, where='family %d' % g)
        centres, doubles = centres + a, doubles + b
    assert centres >= 100 and doubles >= 50
    assert sum(r['stereo']['status'] == M.STEREO_NO_KEKULE for r in got) == 2
    for r in got:
        if r['stereo']['status'] == M.STEREO_NO_KEKULE:
            s = r['stereo']
            assert not (s['atom_parity'].any() or s['atom_label'].any() or s['bond_stereo'].any() or s['bond_label'].any() or s['counts'].any())
            assert s['stereo_key'] == r['rows'].key and r['text']['status'] == M.SMILES_NO_KEKULE and not r['text']['stereo_counts'].any()
    # with all-zero stereo inputs the new entry point writes pg_mol_smiles' bytes
    zero = dataclasses.replace(st, atom_parity=torch.zeros_like(st.atom_parity), bond_stereo=torch.zeros_like(st.bond_stereo))
    plain, blank = M.smiles(res, kekule=st.kekule, capacity=sm.capacity), M.smiles(res, stereo=zero)
    for k in ('text', 'length', 'atom_rank', 'counts', 'status'):
        assert torch.equal(getattr(plain, k), getattr(blank, k)), k
    assert plain.stereo_counts is None and not blank.stereo_counts.any() and not torch.equal(plain.text, sm.text)
    # undefined values (2) are written without a mark
    undef = dataclasses.replace(st, atom_parity=torch.full_like(st.atom_parity, 2), bond_stereo=torch.full_like(st.bond_stereo, 2))
    assert torch.equal(M.smiles(res, stereo=undef).text, plain.text)


def test_renumbered_graphs(family):
    """Under a renumbering of the atoms the multisets of the labels and the stereo key stay, and the new text agrees with the
    coordinates: on every hand example and its mirror image, and on the graphs of the family of which the restatement says that no
    renumbering can move an answer (`numbering_proof`: a double bond is judged on its lowest-index substituents, and the family's
    random coordinates leave many double bonds far from planar)."""
    graphs = T.example_graphs() + [(c, b, np.array(T.mirrored(p), dtype=np.float32)) for c, b, p, _ in T.EXAMPLES.values()]
    graphs += [g for g in family if T.numbering_proof(T.all_rows(*g))]
    assert len(graphs) >= 2 * len(T.EXAMPLES) + 30
    node, pos, edge, sizes = T.batch_from(graphs)
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=23)
    outs = []
    for nd, ps, ed in ((node, pos, edge), (node2, pos2, edge2)):
        res = _result(nd, ps, ed, sizes)
        st = M.stereo(res)
        outs.append(_split(st, M.smiles(res, stereo=st), ps.numpy(), sizes))
    labelled = 0
    for g, (a, b) in enumerate(zip(*outs)):
        _validate(b, where='renumbered %d' % g)
        sa, sb = a['stereo'], b['stereo']
        assert sorted(sa['atom_label'].tolist()) == sorted(sb['atom_label'].tolist()), g
        assert sorted(sa['bond_label'].tolist()) == sorted(sb['bond_label'].tolist()), g
        assert sa['atom_label'].tolist() == sb['atom_label'][perms[g]].tolist(), g          # atom by atom, too
        assert sa['stereo_key'] == sb['stereo_key'] and sa['counts'].tolist() == sb['counts'].tolist() and sa['status'] == sb['status'], g
        assert a['text']['stereo_counts'][[0, 2, 3]].tolist() == b['text']['stereo_counts'][[0, 2, 3]].tolist(), g
        labelled += int((np.abs(sa['atom_label']) == 1).sum() + (np.abs(sa['bond_label']) == 1).sum())
    assert labelled >= 60


def test_rotation_and_translation_change_nothing(family):
    graphs = T.example_graphs() + list(family)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(1.9), -np.sin(1.9)], [0, np.sin(1.9), np.cos(1.9)]])
    moved = [(cl, b, (np.asarray(p, dtype=np.float64) @ rot.T + np.array([3.0, -2.0, 1.0])).astype(np.float32)) for cl, b, p in graphs]
    lim = M.StereoLimits()
    # (by the restatement alone: the graphs whose rounded new coordinates still keep every value MARGIN away from its threshold)
    keep = []
    for g, (cl, b, p) in enumerate(moved):
        r = T.stereo_of(cl, b, p)
        if (all(v is not None and abs(abs(v) - lim.vol_min) > T.MARGIN for v in r['volumes'].values())
                and all(t is not None and abs(abs(t) - lim.planar_min) > T.MARGIN for t in r['planarities'].values())):
            keep.append(g)
    assert len(keep) >= len(graphs) - 3
    _, _, _, before = _run([graphs[g] for g in keep])
    _, _, _, after = _run([moved[g] for g in keep])
    for g, a, b in zip(keep, before, after):
        assert _facts(a) == _facts(b), g


def test_alone_and_inside_a_batch(family):
    pick = [g for g in range(len(family)) if len(family[g][0]) in (9, 10, 64, 65, 128)][:8]
    _, _, _, together = _run([family[g] for g in pick])
    for g, r in zip(pick, together):
        _, _, _, (alone,) = _run([family[g]], capacity=12 * 128)       # (the batch's row width: the same bytes and the same zeros)
        assert _facts(alone) == _facts(r), g
        assert all(np.array_equal(x, y) for x, y in zip(alone['rows'], r['rows'])), g


def test_trajectory_frames_in_one_launch_and_reuse():
    """frames='traj', F = 3 in one launch: the example and its mirror image swapped, then a flat centre and a twisted double bond."""
    (c1, b1, p1, _), (c2, b2, p2, _) = T.EXAMPLES['CHFClBr skeleton'], T.EXAMPLES['cis-1,2-difluoroethene skeleton']
    flat, twisted = [[0, 0, 0], [1, 0, 0], [-0.5, 0.9, 0], [-0.5, -0.9, 0.01]], [p2[0], p2[1], p2[2], [2.0, 0.1, 1.16]]
    frames = [[(c1, b1, p1), (c2, b2, p2)], [(c1, b1, T.mirrored(p1)), (c2, b2, T.EXAMPLES['trans-1,2-difluoroethene skeleton'][2])],
              [(c1, b1, flat), (c2, b2, twisted)]]
    per = [T.batch_from(f) for f in frames]
    sizes = per[0][3]
    traj = tuple(torch.stack([p[k] for p in per]).to(DEV) for k in range(3))
    res = _result(*per[-1][:3], sizes, traj=traj)
    st = M.stereo(res, frames='traj')
    sm = M.smiles(res, frames='traj', stereo=st)
    assert st.status.shape == (3, 2) and st.atom_parity.shape == (3, 8) and sm.text.shape == (3, 2, 96) and sm.stereo_counts.shape == (3, 2, 4)
    for f in range(3):
        for g, r in enumerate(_split(st, sm, per[f][1].numpy(), sizes, f)):
            _validate(r, where='frame %d graph %d' % (f, g))
    assert [sm.strings(f) for f in range(3)] == [['[C@H](F)(Cl)Br', 'F/C=C\\F'], ['[C@@H](F)(Cl)Br', 'F/C=C/F'], ['C(F)(Cl)Br', 'FC=CF']]
    C, Bd = M.STEREO_HAS_CENTRE, M.STEREO_HAS_BOND
    assert st.status.tolist() == [[C, Bd], [C, Bd], [0, 0]] and st.counts[2].tolist() == [[1, 1, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 1]]
    assert st.atom_parity[2].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and st.ok.all()
    # max_undefined: more undefined elements than allowed fail the graph, nothing else changes
    tight = M.stereo(res, frames='traj', screen=st.screen, kekule=st.kekule, rings=st.rings, keys=st.keys, limits=M.StereoLimits(max_undefined=0))
    U = M.STEREO_UNDEFINED
    assert tight.status.tolist() == [[C, Bd], [C, Bd], [U, U]] and tight.ok.tolist() == [[True, True], [True, True], [False, False]]
    assert torch.equal(tight.atom_label, st.atom_label) and torch.equal(tight.stereo_key, st.stereo_key) and tight.screen is st.screen
    # wider thresholds define the flat centre; the final frame alone is the trajectory's last
    wide = M.stereo(res, frames='traj', limits=M.StereoLimits(vol_min=0.01, planar_min=0.001))
    assert abs(int(wide.atom_parity[2, 0])) == 1 and wide.counts[2, 1].tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    final = M.stereo(res)
    assert torch.equal(final.atom_parity[0], st.atom_parity[2]) and torch.equal(final.stereo_key[0], st.stereo_key[2])
    # stages of other frames, or of another result, are refused
    with pytest.raises(ValueError, match='screen'):
        M.stereo(res, frames='final', kekule=st.kekule)
    with pytest.raises(ValueError, match='keys='):
        M.stereo(res, frames='traj', screen=st.screen, keys=final.keys)
    with pytest.raises(ValueError, match='screen'):
        M.smiles(res, stereo=st)
    with pytest.raises(ValueError, match='stereo='):
        M.smiles(res, stereo=st.kekule)
    with pytest.raises(ValueError, match='StereoLimits'):
        M.stereo(res, limits=M.RingLimits())


def test_nonfinite_coordinate_dropped_atom_and_capacity():
    c, b, p, _ = T.EXAMPLES['cis-1,2-difluoroethene skeleton']
    nan = [p[0], p[1], p[2], [float('nan'), 0.0, 0.0]]
    c1, b1, p1, t1 = T.EXAMPLES['CHFClBr skeleton']
    dropped = ([c1[0], 11, c1[1], c1[2], c1[3]], {(0, 2): 1, (0, 3): 1, (0, 4): 1, (0, 1): 1}, [p1[0], [9.0, 9.0, 9.0], p1[1], p1[2], p1[3]])
    _, st, sm, got = _run([(c, b, nan), dropped, (c1, b1, p1)])
    for g, r in enumerate(got):
        _validate(r, where='graph %d' % g)
    assert got[0]['stereo']['status'] == M.STEREO_NONFINITE and got[0]['stereo']['counts'].tolist() == [0, 0, 0, 0, 1, 1, 0, 1]
    assert st.ok.tolist() == [[False, True, True]] and got[0]['text']['text'] == 'FC=CF'
    assert got[1]['text']['text'] == t1 and got[1]['stereo']['atom_parity'].tolist() == [got[2]['stereo']['atom_parity'][0], 0, 0, 0, 0]
    assert got[1]['stereo']['stereo_key'] == got[2]['stereo']['stereo_key']      # a dropped atom has no influence
    # capacity: the needed length passes, one byte fewer is TOO_LONG with the need in the count and the real stereo counts
    graphs = [(c1, b1, p1)]
    _, _, _, (exact,) = _run(graphs, capacity=len(t1))
    _, _, _, (short,) = _run(graphs, capacity=len(t1) - 1)
    _validate(short, capacity=len(t1) - 1)
    assert exact['text']['text'] == t1 and short['text']['status'] == M.SMILES_TOO_LONG | M.SMILES_BRACKET and short['text']['text'] == ''
    assert short['text']['counts'][0] == len(t1) and short['text']['stereo_counts'].tolist() == [1, 0, 0, 0]


def test_cpu_result_and_oversize_graph_are_refused():
    from phoregen_amd import hip
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2

    class Rows:
        cls = atom_parity = charge = torch.zeros(1, n, dtype=torch.int8, device=DEV)
        order = kekule_order = bond_stereo = torch.zeros(1, h, dtype=torch.int8, device=DEV)
        ring_size = torch.zeros(1, h, dtype=torch.uint8, device=DEV)
        hcount = torch.zeros(1, n, dtype=torch.uint8, device=DEV)
        colour = torch.zeros(1, n, dtype=torch.int64, device=DEV)
        key = torch.zeros(1, 1, dtype=torch.int64, device=DEV)
        status = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
        lig_off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        bond_off = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    pos = torch.zeros(n, 3, device=DEV)
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=DEV)   # noqa: E731
    out = dict(status=full((1, 1), torch.int32), counts=full((1, 1, 8), torch.int32), atom_parity=full((1, n), torch.int8),
               atom_label=full((1, n), torch.int8), bond_stereo=full((1, h), torch.int8), bond_label=full((1, h), torch.int8),
               stereo_key=full((1, 1), torch.int64))
    lim = M.StereoLimits()
    with pytest.raises(RuntimeError) as err:
        M._launch_stereo(hip.lib(), pos, 0, Rows, Rows, Rows, Rows, 1, 1, n, lim, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_stereo' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_stereo'):
        M._launch_stereo(hip.lib(), pos, 0, Rows, Rows, Rows, Rows, 1, 1, -1, lim, out)
    with pytest.raises(ValueError, match='stereo'):
        M._launch_stereo(hip.lib(), pos[:5], 0, Rows, Rows, Rows, Rows, 1, 1, n, lim, out)
    sout = dict(status=full((1, 1), torch.int32), counts=full((1, 1, 8), torch.int32), text=full((1, 1, 64), torch.uint8),
                length=full((1, 1), torch.int32), atom_rank=full((1, n), torch.int16), stereo_counts=full((1, 1, 4), torch.int32))
    with pytest.raises(RuntimeError) as err:
        M._launch_smiles(hip.lib(), Rows, Rows, 1, 1, n, M._smiles_table(pos.device), 64, sout, Rows)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_smiles_stereo' in str(err.value)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values()) and all((t == 77).all() for t in sout.values())
    # empty batches return without a launch
    res = _result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])
    empty = M.stereo(res)
    assert empty.status.shape == (1, 0) and empty.atom_parity.shape == (1, 0) and M.smiles(res, stereo=empty).strings() == []


def test_assemble_unique_and_sdf_carry_the_stereo(tmp_path):
    names = ['CHFClBr skeleton', 'meso-tartaric skeleton', 'chiral tartaric skeleton', 'cis-1,2-difluoroethene skeleton',
             'trans-1,2-difluoroethene skeleton']
    graphs = [T.EXAMPLES[k][:3] for k in names] + [(T.EXAMPLES[k][0], T.EXAMPLES[k][1], T.mirrored(T.EXAMPLES[k][2])) for k in names[:3]]
    res, st, sm, got = _run(graphs)
    plain, full = M.assemble(res, keys=True), M.assemble(res, keys=True, stereo=st, smiles=sm, kekule=st.kekule, rings=st.rings)
    for g, (p, m, r) in enumerate(zip(plain, full, got)):
        assert set(m) == set(p) | {'stereo', 'smiles', 'kekule', 'rings'}
        for name in p:
            assert torch.equal(p[name], m[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], m[name]), name
        s, want = m['stereo'], T.assembled(*graphs[g])['stereo']
        assert set(s) == set(want) == {'status', 'stereo_ok', 'stereo_key', 'atom_parity', 'atom_label', 'bond_stereo', 'bond_label'} | set(M.STEREO_COUNTS)
        assert all(np.array_equal(s[k], want[k]) for k in want), g
        assert s['atom_parity'].dtype == np.int8 and len(s['bond_label']) == len(m['bond_type']) and isinstance(s['stereo_key'], int)
        assert m['smiles']['text'] == r['text']['text'] and [m['smiles'][k] for k in M.SMILES_STEREO_COUNTS] == r['text']['stereo_counts'].tolist()
    # identity: the mirror pair is one molecule without stereo and two with it; the meso pair is one either way
    assert M.unique_molecules(full)[1] == [0, 1, 1, 2, 2, 0, 1, 1]
    assert M.unique_molecules(full, stereo=True)[1] == [0, 1, 2, 3, 4, 5, 1, 6]
    assert M.duplicate_groups(st.stereo_key[0])[2].tolist() == [0, 1, 2, 3, 4, 5, 1, 6]
    assert M.same_molecule(full[0], full[5]) and not M.same_molecule(full[0], full[5], stereo=True) and M.same_molecule(full[1], full[6], stereo=True)
    path = tmp_path / 's.sdf'
    M.write_sdf(str(path), full)
    text = path.read_text()
    assert text.count('> <PHOREGEN_STEREO>') == 8 and 'stereo_key %016x\n' % full[0]['stereo']['stereo_key'] in text
    assert '> <PHOREGEN_SMILES>\n[C@H](F)(Cl)Br\n\n> <PHOREGEN_STEREO>\nstatus 0x04\n' in text and text.startswith(M.mol_block(full[0]))
    with pytest.raises(ValueError, match='stereo='):                    # of another result
        M.assemble(res, stereo=M.stereo(_result(*T.batch_from(graphs[:1])[:3], [4])))


def test_sample_valid_and_cli_with_stereo(tmp_path):
    """A stand-in model that hands out the CHFClBr skeleton, its mirror image and the cis skeleton in turn: with stereo= the mirror
    images are different molecules, without it one."""
    parts = [T.batch_from([g]) for g in (T.EXAMPLES['CHFClBr skeleton'][:3],
                                         (*T.EXAMPLES['CHFClBr skeleton'][:2], T.mirrored(T.EXAMPLES['CHFClBr skeleton'][2])),
                                         T.EXAMPLES['cis-1,2-difluoroethene skeleton'][:3])]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % 3] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [p[3][0] for p in pick])
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=3, unique=True, stereo=True, smiles=True)
    assert [m['smiles']['text'] for m in out['finished']] == ['[C@H](F)(Cl)Br', '[C@@H](F)(Cl)Br', 'F/C=C\\F'] and not out['duplicates']
    assert all(m['stereo']['stereo_ok'] and 'kekule' not in m for m in out['finished'])
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=3, unique=True, smiles=True, max_failed_factor=1)
    assert [m['smiles']['text'] for m in out['finished']] == ['C(F)(Cl)Br', 'FC=CF'] and len(out['duplicates']) >= 1
    out = M.sample_valid(Rota(), None, num_samples=2, batch_size=3, unique=True, stereo=M.StereoLimits(vol_min=3.5), max_failed_factor=2)
    assert [m['stereo']['atom_parity'].tolist() for m in out['finished']] == [[2, 0, 0, 0], [0, 0, 0, 0]] and len(out['duplicates']) >= 1
    # the command-line tool: isomeric lines, the data item, the stereo keys
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    outdir = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(outdir), '--smiles', '--stereo', '--unique', '--sdf', '--num_steps', '10',
                          '--stereo_limits', '{"vol_min": 0.4}'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(outdir.glob('*.pt'))), weights_only=False)
    lines = next(outdir.glob('*_SMILES_all.txt')).read_text().split('\n')
    assert lines[:-1] == [m['smiles']['text'] for m in done] and all(m['stereo']['stereo_ok'] for m in done)
    assert next(outdir.glob('*_keys.txt')).read_text().split('\n')[:-1] == ['%016x' % m['stereo']['stereo_key'] for m in done]
    for m in done:
        atoms, bonds, centres, _ = T.read_isomeric(m['smiles']['text'])
        assert len(atoms) == len(m['element']) and len(centres) == int((np.abs(m['stereo']['atom_parity']) == 1).sum())
    sdfs = sorted((outdir / 'sdf_results').glob('*.sdf'))
    assert len(sdfs) == len(done) and all('> <PHOREGEN_STEREO>' in p.read_text() for p in sdfs)
