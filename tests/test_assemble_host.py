"""CPU: the carrying side of phoregen_amd/molecule.py without a device -- `assemble` on hand-made holders of every analysis (nothing is
launched when every holder is handed in), the order of the blob's parts, the order of the record list, and the verdicts `sample_valid`
filters on.  The holders hold seeded random values: what is checked is where `assemble` cuts and how it slices, not chemistry."""
import copy

import numpy as np
import pytest
import torch

from phoregen_amd import hydrogens as HY, molecule as M, substructure as SUB

SIZES = [3, 1, 5, 0, 4]          # a graph without atoms, one without pairs; every larger one loses an atom and lacks a bond
KEY_ORDER = ['geom', 'rings', 'kekule', 'features', 'smiles', 'stereo', 'fingerprint', 'fp_bits', 'fp_radius', 'substructure',
             'substructure_ok', 'hydrogens']
BASE_KEYS = ['element', 'atom_pos', 'bond_index', 'bond_type', 'status', 'valid', 'n_components', 'valence']


def seeded(mods=(M, SUB, HY), sizes=SIZES, seed=0, stereo_counts=True):
    """(result, screen with `agree`, {assemble keyword: holder}, MolKeys) on the CPU for graphs of `sizes` atoms, from one seed.
    mods: the molecule, substructure and hydrogens modules whose classes the holders are made of."""
    M, SUB, HY = mods
    rng = np.random.default_rng(seed)
    B, N, H = len(sizes), sum(sizes), sum(n * (n - 1) // 2 for n in sizes)

    def ints(dtype, lo, hi, *shape):
        return torch.from_numpy(rng.integers(lo, hi, size=(1,) + shape).astype(dtype))

    def reals(*shape):
        return torch.from_numpy(rng.uniform(0.5, 9.5, size=(1,) + shape).astype(np.float32))

    def head(n_counts):
        st = ints(np.int32, 0, 64, B)
        return dict(status=st, counts=ints(np.int32, 0, 1000, B, n_counts), ok=st % 2 == 0)

    def offsets(per_graph):
        return torch.tensor(np.concatenate([[0], np.cumsum(per_graph)]), dtype=torch.int32)

    cls, compact, order, ring_sys = (np.zeros(N, np.int8), np.zeros(N, np.int16), np.zeros(H, np.int8), np.zeros(N, np.int16))
    n0 = h0 = 0
    for n in sizes:
        c = rng.integers(0, 11, size=n)
        if n >= 3:
            c[rng.integers(0, n)] = -1                                 # a dropped atom
        kept = np.nonzero(c >= 0)[0]
        cls[n0:n0 + n], compact[n0:n0 + n] = c, -1
        compact[n0 + kept] = np.arange(kept.size)
        ring_sys[n0:n0 + n] = rng.integers(-1, max(n, 1), size=n)      # -1 or a local atom index
        a, b = np.triu_indices(n, 1)
        between_kept = np.nonzero((c[a] >= 0) & (c[b] >= 0))[0]
        o = np.zeros(a.size, np.int8)
        o[between_kept] = rng.integers(0, 5, size=between_kept.size)
        if between_kept.size:
            o[between_kept[0]] = 2                                     # a bond,
        if between_kept.size > 1:
            o[between_kept[-1]] = 0                                    # and a pair of kept atoms without one
        order[h0:h0 + a.size] = o
        n0, h0 = n0 + n, h0 + a.size
    status = ints(np.int32, 0, 64, B)
    sc = M.Screen(status=status, counts=ints(np.int32, 0, 9, B, 4), valid=(status & M.FAIL_MASK) == 0, cls=torch.from_numpy(cls)[None],
                  compact=torch.from_numpy(compact)[None], valence2=ints(np.uint8, 0, 9, N), comp=ints(np.int16, 0, 3, N),
                  order=torch.from_numpy(order)[None], lig_off=offsets(sizes), bond_off=offsets([n * (n - 1) for n in sizes]),
                  num_atoms=list(sizes), bonds='distance', agree=ints(np.int32, 0, 50, B, len(M.BOND_AGREE_COUNTS)))
    res = {'pred': [torch.zeros(N, 12), reals(N, 3)[0], torch.zeros(2 * H, 6)]}
    points = rng.integers(0, 4, size=B)                                # points per graph, some without any
    points[0] = 2
    Q, off = int(points.sum()), offsets(points)
    dist = reals(Q)
    dist[0, 0] = float('inf')
    mk = M.MolKeys(key=ints(np.int64, -2 ** 63, 2 ** 63, B), colour=ints(np.int64, -2 ** 63, 2 ** 63, N))
    geo = M.Geometry(**dict(head(6), metrics=reals(B, 8)), point_dist=dist, point_atom=ints(np.int16, -1, 3, Q), point_off=off,
                     point_range=torch.stack([off[:-1], off[1:]], 1).contiguous(), limits=M.GeomLimits(), screen=sc)
    rg = M.Rings(**head(len(M.RING_COUNTS)), ring_size=ints(np.uint8, 0, 9, H), atom_ring=ints(np.uint8, 0, 9, N),
                 ring_sys=torch.from_numpy(ring_sys)[None], limits=M.RingLimits(), screen=sc)
    kek = M.Kekule(**head(len(M.KEKULE_COUNTS)), kekule_order=ints(np.int8, 1, 4, H), hcount=ints(np.uint8, 0, 4, N),
                   charge=ints(np.int8, 0, 2, N), options=M.KekuleOptions(), screen=sc)
    feat = M.Features(**head(len(M.FEATURE_COUNTS)), atom_fp=ints(np.uint8, 0, 128, N), point_dist=reals(Q) - 0.4,
                      point_atom=ints(np.int16, -1, 3, Q), point_off=off, point_range=geo.point_range + 1,
                      point_kind=ints(np.int8, -2, 7, Q + 1)[0], limits=M.FeatureLimits(), screen=sc, kekule=kek, rings=rg)
    parity, cis = ints(np.int8, -1, 3, N), ints(np.int8, -1, 3, H)
    flip = lambda p: torch.where(p.abs() == 1, p * (ints(np.int8, 0, 2, p.size(1)) * 2 - 1), p)          # noqa: E731  (a label: 0 and 2 as they are)
    st = M.Stereo(**head(len(M.STEREO_COUNTS)), atom_parity=parity, atom_label=flip(parity), bond_stereo=cis, bond_label=flip(cis),
                  stereo_key=ints(np.int64, -2 ** 63, 2 ** 63, B),
                  limits=M.StereoLimits(), screen=sc, kekule=kek, rings=rg, keys=mk)
    cap = 24
    smi = M.Smiles(**dict(head(len(M.SMILES_COUNTS)), status=torch.tensor([0, 8, 1, 16, 32], dtype=torch.int32).repeat(B // 5 + 1)[None, :B]),
                   text=ints(np.uint8, 65, 91, B, cap), length=ints(np.int32, 0, cap + 1, B), atom_rank=ints(np.int16, -1, 5, N), capacity=cap,
                   screen=sc, kekule=kek, stereo_counts=ints(np.int32, 0, 9, B, 4) if stereo_counts else None, stereo=st if stereo_counts else None)
    fps = M.Fingerprints(fp=ints(np.int64, -2 ** 63, 2 ** 63, B, M.FP_WORDS), bits=ints(np.int32, 0, 99, B), radius=3, screen=sc)
    patterns = [SUB.Pattern('one', (SUB.QueryAtom(),)), SUB.Pattern('pair', (SUB.QueryAtom(), SUB.QueryAtom()), (SUB.QueryBond(0, 1),), min=1)]
    sub_status = ints(np.int32, 0, 16, B, 2)
    sub = SUB.Substructure(embeddings=ints(np.int32, 0, 9, B, 2), anchors=ints(np.int32, 0, 9, B, 2), atom_mask=ints(np.int64, 0, 32, B, 2, 2),
                           first=ints(np.int16, -1, 4, B, 2, SUB.MAX_ATOMS), status=sub_status, ok=((sub_status & SUB.SUB_OUT_OF_BOUNDS) == 0).all(-1),
                           patterns=patterns, max_steps=SUB.DEFAULT_STEPS, screen=sc, rings=rg, kekule=kek)
    contact = reals(B)
    contact[0, -1] = float('inf')
    hyd = HY.Hydrogens(**head(len(HY.HYD_COUNTS)), h_pos=reals(N, HY.MAX_PER_ATOM, 3), h_placed=ints(np.uint8, 0, HY.MAX_PER_ATOM + 1, N),
                       site_shape=ints(np.uint8, 0, 5, N), min_contact=contact, options=HY.HydrogenOptions(), screen=sc, kekule=kek)
    return res, sc, dict(geometry=geo, rings=rg, kekule=kek, features=feat, smiles=smi, stereo=st, fingerprints=fps, substructure=sub,
                         hydrogens=hyd), mk


def same(a, b):
    """Deep equality: types, dict key order, arrays and tensors by dtype, shape and content (bit for bit)."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


@pytest.fixture(scope='module')
def made():
    """Built once, read by several tests, changed by none."""
    return seeded()


def test_the_seeded_graphs_have_the_edge_cases(made):
    _, sc, _, _ = made
    cls, order = sc.cls[0].numpy(), sc.order[0].numpy()
    assert 0 in SIZES and 1 in SIZES
    n0 = h0 = 0
    for n in SIZES:
        h = n * (n - 1) // 2
        if n >= 3:
            assert (cls[n0:n0 + n] < 0).sum() == 1 and (order[h0:h0 + h] != 0).any() and (order[h0:h0 + h] == 0).any()
        n0, h0 = n0 + n, h0 + h


@pytest.mark.parametrize('with_screen', [False, True])
@pytest.mark.parametrize('with_keys', [False, True])
def test_an_entry_does_not_depend_on_its_company(made, monkeypatch, with_screen, with_keys):
    """Every analysis adds the same entries alone and together with all the others, and the base keys are the same in both: a part
    cut at another part's offset, or a view reshaped with another analysis's width, changes one of the two."""
    res, sc, holders, mk = made
    monkeypatch.setattr(M, 'molecule_keys', lambda screen: mk)
    monkeypatch.setattr(M, '_screen', lambda results, frames: sc)      # (only the call without a holder or a screen computes one)
    common = dict(keys=with_keys, **({'screen': sc} if with_screen else {}))
    base = BASE_KEYS + (['bonds', 'bond_agreement'] if with_screen else []) + (['key', 'atom_colour'] if with_keys else [])
    bare, full = M.assemble(res, **common), M.assemble(res, **holders, **common)
    assert len(bare) == len(full) == len(SIZES)
    for m, q in zip(bare, full):
        assert list(m) == base and list(q) == base + KEY_ORDER and same(m, {k: q[k] for k in base})
    assert [len(m['element']) for m in bare] == [2, 1, 4, 0, 3]
    if with_screen:
        assert all(m['bonds'] == 'distance' and list(m['bond_agreement']) == list(M.BOND_AGREE_COUNTS) for m in bare)
    seen = []
    for keyword, x in holders.items():
        alone = M.assemble(res, **{keyword: x}, **common)
        added = [k for k in alone[0] if k not in base]
        seen += added
        for m, q in zip(alone, full):
            assert list(m) == base + added and same(m, {k: q[k] for k in m})
    assert seen == KEY_ORDER


def test_the_parts_are_ordered_widest_first(made):
    res, sc, holders, mk = made
    parts = M._blob_parts(res['pred'][1], sc, mk, True, M._handed(holders))
    widths = [np.dtype(dt).itemsize for _, _, dt in parts]
    assert widths == sorted(widths, reverse=True) and set(widths) == {8, 4, 2, 1}
    assert len({name for name, _, _ in parts}) == len(parts) > 50
    assert all(t.element_size() == w for (_, t, _), w in zip(parts, widths))


def test_the_record_list_names_every_keyword_once_and_in_order(made):
    keywords = [a.keyword for a in M._ANALYSES]
    assert keywords == ['geometry', 'rings', 'kekule', 'features', 'smiles', 'stereo', 'fingerprints', 'substructure', 'hydrogens']
    assert [rec.keyword for rec in M._analyses(lambda a: True)] == keywords == list(made[2])
    assert [a.key for a in M._ANALYSES] == [k for k in KEY_ORDER if k not in ('fp_bits', 'fp_radius', 'substructure_ok')]
    assert SUB.ANALYSIS.holder is SUB.Substructure and HY.ANALYSIS.holder is HY.Hydrogens and HY.ANALYSIS.also == ('kekule',)


def test_write_sdf_writes_the_items_in_their_order(made, tmp_path):
    res, sc, holders, mk = made
    path = tmp_path / 'all.sdf'
    M.write_sdf(str(path), [M.assemble(res, screen=sc, **holders)[2]])
    tags = [ln[3:-1] for ln in path.read_text().split('\n') if ln.startswith('> <')]
    assert tags == ['PHOREGEN_' + t for t in ('BONDS', 'GEOM', 'RINGS', 'KEKULE', 'FEATURES', 'STEREO', 'FINGERPRINT', 'SUBSTRUCTURE', 'HYDROGENS')]


ALL_OK = {'valid': True, 'geom': {'geom_ok': True}, 'rings': {'rings_ok': True}, 'kekule': {'kekule_ok': True},
          'features': {'features_ok': True}, 'smiles': {'smiles_ok': True}, 'stereo': {'stereo_ok': True}, 'substructure_ok': True,
          'hydrogens': {'hydrogens_ok': True}}
VERDICTS = [('geometry', (None, None, M.GeomLimits()), ('geom', 'geom_ok')), ('rings', True, ('rings', 'rings_ok')),
            ('kekule', M.KekuleOptions(allow_charged=False), ('kekule', 'kekule_ok')),
            ('features', (None, None, M.FeatureLimits()), ('features', 'features_ok')), ('smiles', True, ('smiles', 'smiles_ok')),
            ('stereo', True, ('stereo', 'stereo_ok')), ('substructure', [SUB.Pattern('one', (SUB.QueryAtom(),))], ('substructure_ok',)),
            ('hydrogens', True, ('hydrogens', 'hydrogens_ok'))]


def _without(path):
    m = copy.deepcopy(ALL_OK)
    (m[path[0]] if len(path) == 2 else m)[path[-1]] = False
    return m


class _Rota:
    def __init__(self, mols):
        self.mols, self.i = mols, 0

    def sample(self, data, n, device, **kw):
        self.i += n
        return [self.mols[(self.i - n + j) % len(self.mols)] for j in range(n)]


@pytest.fixture
def no_device(monkeypatch):
    """`sample_valid` with `assemble` and every entry point replaced: the molecules are the model's, the keywords are recorded."""
    seen = []

    def assemble(res, keys=False, **kw):
        seen.append(kw)
        return res
    monkeypatch.setattr(M, 'assemble', assemble)
    monkeypatch.setattr(M, '_screen', lambda res, frames: 'screen')
    monkeypatch.setattr(M, 'molecule_keys', lambda sc: 'keys')
    monkeypatch.setattr(M, '_geometry', lambda res, pp, ex, screen, limits: ('geometry', limits))
    monkeypatch.setattr(M, '_rings', lambda res, screen, limits: ('rings', limits))
    monkeypatch.setattr(M, '_kekulize', lambda res, screen, options: ('kekule', options))
    monkeypatch.setattr(M, '_features', lambda res, pp, pk, screen, kekule, rings, limits: ('features', kekule, rings, limits))
    monkeypatch.setattr(M, '_smiles', lambda res, screen, kekule, stereo: ('smiles', kekule, stereo))
    monkeypatch.setattr(M, '_stereo', lambda res, screen, kekule, rings, keys, limits: ('stereo', kekule, rings, keys, limits))
    monkeypatch.setattr(SUB, 'substructure', lambda res, patterns, screen, rings, kekule, max_steps: ('substructure', rings, kekule, max_steps))
    monkeypatch.setattr(HY, 'hydrogens', lambda res, screen, kekule, options: ('hydrogens', kekule, options))
    return seen


@pytest.mark.parametrize('keyword, value, path', VERDICTS, ids=[v[0] for v in VERDICTS])
def test_sample_valid_filters_on_the_verdict_of_what_was_asked_for(no_device, keyword, value, path):
    bad, good = _without(path), copy.deepcopy(ALL_OK)
    out = M.sample_valid(_Rota([bad, good]), None, num_samples=1, **{keyword: value})
    assert out['failed'] == [bad] and out['finished'] == [good] and out['failed'][0] is bad and out['n_calls'] == 2
    assert all(set(kw) == {keyword} | ({'kekule'} if keyword == 'hydrogens' else set()) for kw in no_device) and len(no_device) == 2
    # a verdict that was not asked for does not count: the next analysis's (never the Kekulé form's after hydrogens=)
    other = _without(VERDICTS[([v[0] for v in VERDICTS].index(keyword) + 1) % len(VERDICTS)][2])
    out = M.sample_valid(_Rota([other]), None, num_samples=1, **{keyword: value})
    assert out['finished'] == [other] and out['failed'] == []


def test_sample_valid_without_an_analysis_filters_on_valid_alone(no_device):
    nothing_ok = {k: ({kk: False for kk in v} if isinstance(v, dict) else k == 'valid') for k, v in ALL_OK.items()}
    invalid = dict(copy.deepcopy(ALL_OK), valid=False)
    out = M.sample_valid(_Rota([invalid, nothing_ok]), None, num_samples=1)
    assert out['failed'] == [invalid] and out['finished'] == [nothing_ok] and no_device == [{}, {}]


def test_sample_valid_hydrogens_carry_and_filter_on_the_kekule_form(no_device):
    bad, good = _without(('kekule', 'kekule_ok')), copy.deepcopy(ALL_OK)
    out = M.sample_valid(_Rota([bad, good]), None, num_samples=1, hydrogens=True)
    assert out['failed'] == [bad] and out['finished'] == [good]
    kek = ('kekule', M.KekuleOptions())                                 # the default options, computed once and shared
    assert no_device == [{'kekule': kek, 'hydrogens': ('hydrogens', kek, HY.HydrogenOptions())}] * 2
    del no_device[:]
    mine = M.KekuleOptions(allow_charged=False)                        # with kekule= too: the user's options
    M.sample_valid(_Rota([good]), None, num_samples=1, hydrogens=True, kekule=mine)
    assert no_device == [{'kekule': ('kekule', mine), 'hydrogens': ('hydrogens', ('kekule', mine), HY.HydrogenOptions())}]


def test_sample_valid_takes_what_an_analysis_needs_from_the_draw(no_device):
    good = copy.deepcopy(ALL_OK)
    limits = M.RingLimits(ring_min=5)
    M.sample_valid(_Rota([good]), None, num_samples=1, smiles=True, stereo=True, rings=limits, substructure=([SUB.Pattern('one', (SUB.QueryAtom(),))], 7))
    kek, rg = ('kekule', M.KekuleOptions()), ('rings', limits)
    st = ('stereo', kek, rg, 'keys', M.StereoLimits())
    assert no_device == [{'rings': rg, 'smiles': ('smiles', kek, st), 'stereo': st, 'substructure': ('substructure', rg, kek, 7)}]
