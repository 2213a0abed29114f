"""Plain restatement of the substructure search (DESIGN.md 2.9 "Substructure"; phoregen_amd/substructure.py, csrc/mol_sub.hip) for the
tests, written from the definition: a recursive search over dicts and lists, no bit sets, no explicit stack, no device code.  It reads
patterns in the dict form of `Pattern.from_dict` with a parser of its own and shares nothing with the product but named constants
(the status bits, the limits, the element symbols).  Also here: the pattern lists of the tests and the yardstick, networkx's
`GraphMatcher.subgraph_monomorphisms_iter` (tests only; the product does not import networkx)."""
import numpy as np

from phoregen_amd import molecule as M
from phoregen_amd import substructure as S
from phoregen_amd.utils.sample_utils import ATOM_TYPES

import kekule_reference as K
import mol_support as MS
import molkey_reference as Q
import ring_reference as G

SYMBOL_CLASS = {M.ELEMENT_SYMBOL[z]: c for c, z in enumerate(ATOM_TYPES)}
STEP_LIMIT = 5_000_000               # the restatement gives up (raises) beyond this many steps of one root: no test needs more


# ---- targets ---------------------------------------------------------------------------------------------------------------------
def target_of_rows(cls, order, ring_size, atom_ring, hcount=None, charge=None, kekule_status=0):
    """One graph as the screen, the ring screen and the Kekulé kernel wrote it -> {'atoms': [property dict per kept atom, in compact
    numbering], 'bonds': {(a, b): (order, ring bond)} both ways, 'nbr': sorted neighbours per atom, 'kekule_failed', 'local': local index per compact index}."""
    w = MS.pair_walk(cls, order)
    kept = [i for i, k in enumerate(w.kept) if k]
    compact = {i: c for c, i in enumerate(kept)}
    atoms = [{'cls': int(cls[i]), 'degree': 0, 'hcount': int(hcount[i]) if hcount is not None else 0,
              'charge': int(charge[i]) if charge is not None else 0, 'ring': int(atom_ring[i]) > 0, 'aromatic': False} for i in kept]
    bonds = {}
    for (a, b), row in w.rows.items():
        ca, cb = compact[a], compact[b]
        bonds[(ca, cb)] = bonds[(cb, ca)] = (w.order[row], int(ring_size[row]) > 0)
        for x in (ca, cb):
            atoms[x]['degree'] += 1
            atoms[x]['aromatic'] = atoms[x]['aromatic'] or w.order[row] == 4
    nbr = [sorted(b for (a, b) in bonds if a == c) for c in range(len(kept))]
    return {'atoms': atoms, 'bonds': bonds, 'nbr': nbr, 'kekule_failed': bool(int(kekule_status) & M.KEKULE_FAILED), 'local': kept}


def target_of_classes(classes, bonds, kekule=True):
    """A target from atom classes 0..11 and {(a, b): bond class 1..5}, properties from ring_reference / kekule_reference."""
    cls, order = MS.rows_of(list(classes), dict(bonds))
    rings = G.rings_of_rows(cls, order)
    if not kekule:
        return target_of_rows(cls, order, rings['ring_size'], rings['atom_ring'])
    kek = K.kekule_of_rows(cls, order)
    return target_of_rows(cls, order, rings['ring_size'], rings['atom_ring'], kek['hcount'], kek['charge'], kek['status'])


def target_of_mol(m, kekule=True):
    """A target from an assembled-style dict ('element', 'bond_index', 'bond_type')."""
    bi, bt = np.asarray(m['bond_index']).reshape(2, -1), np.asarray(m['bond_type']).reshape(-1)
    return target_of_classes([ATOM_TYPES.index(int(z)) for z in m['element']],
                             {(int(min(a, b)), int(max(a, b))): int(t) for a, b, t in zip(bi[0], bi[1], bt)}, kekule)


# ---- patterns (the dict form) -------------------------------------------------------------------------------------------------------
def parse(p):
    """{'k', 'atoms': [constraint dict with 'elements' as a set of classes], 'bond': {(a, b): (orders, ring)} both ways, 'order',
    'uses_kekule', 'min', 'max'} of a pattern dict."""
    atoms = []
    for a in p['atoms']:
        el = a.get('elements')
        el = set(range(11)) if el is None else {SYMBOL_CLASS[e] if isinstance(e, str) else ATOM_TYPES.index(e) for e in el}

        def rng(v):
            return (0, 255) if v is None else (v, v) if isinstance(v, int) else tuple(v)
        atoms.append({'elements': el, 'degree': rng(a.get('degree')), 'hcount': rng(a.get('hcount')), 'charge': a.get('charge'),
                      'ring': a.get('ring'), 'aromatic': a.get('aromatic')})
    k = len(atoms)
    bond, nbr = {}, [[] for _ in range(k)]
    for b in p.get('bonds', ()):
        c = (set(b.get('orders') or (1, 2, 3, 4)), b.get('ring'))
        bond[(b['a'], b['b'])] = bond[(b['b'], b['a'])] = c
        nbr[b['a']].append(b['b'])
        nbr[b['b']].append(b['a'])
    order, front = [0], [0]                                            # breadth-first from atom 0, neighbours ascending
    while front:
        nxt = []
        for u in front:
            for v in sorted(nbr[u]):
                if v not in order:
                    order.append(v)
                    nxt.append(v)
        front = nxt
    assert len(order) == k, 'a disconnected pattern'
    return {'k': k, 'atoms': atoms, 'bond': bond, 'order': order, 'min': p.get('min') or 0, 'max': p.get('max'),
            'uses_kekule': any(a.get('hcount') is not None or a.get('charge') is not None for a in p['atoms'])}


def atom_meets(q, t):
    return (t['cls'] in q['elements'] and q['degree'][0] <= t['degree'] <= q['degree'][1] and q['hcount'][0] <= t['hcount'] <= q['hcount'][1]
            and (q['charge'] is None or q['charge'] == t['charge']) and (q['ring'] is None or q['ring'] == t['ring'])
            and (q['aromatic'] is None or q['aromatic'] == t['aromatic']))


def bond_meets(qb, tb):
    return tb is not None and tb[0] in qb[0] and (qb[1] is None or qb[1] == tb[1])


def is_embedding(target, p, emb):
    """The definition, on one candidate: emb[q] = the image of query atom q."""
    pat = parse(p) if 'order' not in p else p
    emb = list(emb)
    if len(emb) != pat['k'] or len(set(emb)) != len(emb) or any(not 0 <= t < len(target['atoms']) for t in emb):
        return False
    if pat['uses_kekule'] and target['kekule_failed']:
        return False
    return (all(atom_meets(pat['atoms'][q], target['atoms'][emb[q]]) for q in range(pat['k']))
            and all(bond_meets(qb, target['bonds'].get((emb[a], emb[b]))) for (a, b), qb in pat['bond'].items()))


# ---- the search -----------------------------------------------------------------------------------------------------------------------
def search(target, p, max_steps=S.DEFAULT_STEPS):
    """Every output of the definition for one (graph, pattern), untruncated: 'embeddings' (the count), 'all' (the embeddings per query
    atom, in the defined order), 'anchors', 'mask' (an int, bit c = compact atom c), 'first' (16 entries), 'steps' {root: steps(r)} over
    the admissible roots, 'truncated' (some steps(r) > max_steps), 'no_kekule' and 'status' (for the untruncated values)."""
    pat = parse(p)
    k, order, atoms, bonds = pat['k'], pat['order'], target['atoms'], target['bonds']
    found, steps = [], {}
    no_kekule = pat['uses_kekule'] and target['kekule_failed']

    def extend(image, root):
        d = len(image)
        if d == k:
            found.append(tuple(image))
            return
        q = order[d]
        earlier = [e for e in range(d) if (q, order[e]) in pat['bond']]          # earlier[0] is the walk parent
        for t in target['nbr'][image[earlier[0]]]:                    # (ascending; only a neighbour of the parent's image can pass)
            if t in image or not atom_meets(pat['atoms'][q], atoms[t]):
                continue
            if not bond_meets(pat['bond'][(q, order[earlier[0]])], bonds.get((t, image[earlier[0]]))):
                continue
            steps[root] += 1                                           # one way to go on along the walk
            if steps[root] > STEP_LIMIT:
                raise RuntimeError('sub_reference.search: more steps than the restatement is meant for')
            if all(bond_meets(pat['bond'][(q, order[e])], bonds.get((t, image[e]))) for e in earlier[1:]):
                extend(image + [t], root)

    if not no_kekule:
        for r in range(len(atoms)):
            if atom_meets(pat['atoms'][0], atoms[r]):
                steps[r] = 0
                extend([r], r)
    every = []
    for image in found:                                                # positions -> query atoms
        emb = [0] * k
        for d, t in enumerate(image):
            emb[order[d]] = t
        every.append(tuple(emb))
    mask = 0
    for emb in every:
        for t in emb:
            mask |= 1 << t
    anchors = len({emb[0] for emb in every})
    truncated = any(s > max_steps for s in steps.values())
    bounded = pat['min'] > 0 or pat['max'] is not None
    out = anchors < pat['min'] or (pat['max'] is not None and anchors > pat['max']) or (bounded and truncated)
    status = ((S.SUB_MATCHED if every else 0) | (S.SUB_NO_KEKULE if no_kekule else 0) | (S.SUB_TRUNCATED if truncated else 0)
              | (S.SUB_OUT_OF_BOUNDS if out else 0))
    first = (list(every[0]) if every else []) + [-1] * (S.MAX_ATOMS - (k if every else 0))
    return {'embeddings': min(len(every), 2 ** 31 - 1), 'all': every, 'anchors': anchors, 'mask': mask, 'first': first, 'steps': steps,
            'truncated': truncated, 'no_kekule': bool(no_kekule), 'status': status, 'bounded': bounded}


def mask_words(mask):
    return [mask & (1 << 64) - 1, mask >> 64]


# ---- the yardstick: networkx ------------------------------------------------------------------------------------------------------
def nx_count(target, p):
    """The number of monomorphisms of the pattern into the target by networkx, with the same node and edge predicates."""
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
    pat = parse(p)
    if pat['uses_kekule'] and target['kekule_failed']:
        return 0
    big, small = nx.Graph(), nx.Graph()
    for i, a in enumerate(target['atoms']):
        big.add_node(i, t=a)
    for (a, b), v in target['bonds'].items():
        big.add_edge(a, b, t=v)
    for q, a in enumerate(pat['atoms']):
        small.add_node(q, q=a)
    for (a, b), v in pat['bond'].items():
        small.add_edge(a, b, q=v)
    gm = GraphMatcher(big, small, node_match=lambda t, q: atom_meets(q['q'], t['t']), edge_match=lambda t, q: bond_meets(q['q'], t['t']))
    return sum(1 for _ in gm.subgraph_monomorphisms_iter())


# ---- the tests' pattern lists ---------------------------------------------------------------------------------------------------------
def _path(n):
    return [{'a': a, 'b': b} for a, b in MS.chain(n, 0)]


def _cycle(n, **kw):
    return [dict({'a': a, 'b': b}, **kw) for a, b in MS.cycle(n, 0)]


_DECALIN = _cycle(6) + [{'a': 0, 'b': 6}, {'a': 6, 'b': 7}, {'a': 7, 'b': 8}, {'a': 8, 'b': 9}, {'a': 1, 'b': 9}]

PATTERNS = [
    {'name': 'any-atom', 'atoms': [{}]},
    {'name': 'C-O', 'atoms': [{'elements': ['C']}, {'elements': ['O']}], 'bonds': [{'a': 0, 'b': 1, 'orders': [1]}]},
    {'name': 'C=any', 'atoms': [{'elements': ['C']}, {}], 'bonds': [{'a': 0, 'b': 1, 'orders': [2]}]},
    {'name': 'path-4', 'atoms': [{}] * 4, 'bonds': _path(4)},
    {'name': 'path-8', 'atoms': [{}] * 8, 'bonds': _path(8)},
    {'name': 'path-16', 'atoms': [{}] * 16, 'bonds': _path(16)},
    {'name': '5-cycle', 'atoms': [{}] * 5, 'bonds': _cycle(5)},
    {'name': '6-cycle', 'atoms': [{}] * 6, 'bonds': _cycle(6)},
    {'name': 'aromatic-ring', 'atoms': [{'elements': ['C']}] * 6, 'bonds': _cycle(6, orders=[4])},
    {'name': '3-star', 'atoms': [{'elements': ['C']}, {}, {}, {}], 'bonds': [{'a': 0, 'b': i} for i in (1, 2, 3)]},
    {'name': 'NO-C-NO', 'atoms': [{'elements': ['C']}, {'elements': ['N', 'O']}, {'elements': ['N', 'O']}],
     'bonds': [{'a': 0, 'b': 1}, {'a': 0, 'b': 2}]},
    {'name': 'fused-bicycle', 'atoms': [{}] * 10, 'bonds': _DECALIN},
]

# constraints on degree, ring, aromatic, hcount, charge and the bond ring flag; the first four carry bounds on `anchors`
PROPERTY_PATTERNS = [
    {'name': 'ring-fusion-atom', 'atoms': [{'degree': 3, 'ring': True}], 'min': 1},
    {'name': 'bridge-bond', 'atoms': [{'ring': True}, {'ring': True}], 'bonds': [{'a': 0, 'b': 1, 'ring': False}], 'max': 0},
    {'name': 'ring-bond', 'atoms': [{}, {}], 'bonds': [{'a': 0, 'b': 1, 'ring': True}], 'min': 1, 'max': 20},
    {'name': 'aromatic-N', 'atoms': [{'elements': ['N'], 'aromatic': True}], 'max': 1},
    {'name': 'CH2', 'atoms': [{'elements': ['C'], 'hcount': 2}]},
    {'name': 'OH', 'atoms': [{'elements': ['O'], 'hcount': [1, 2], 'degree': [0, 1]}, ], 'min': 0},
    {'name': 'cation', 'atoms': [{'charge': 1}]},
    {'name': 'neutral-chain-C', 'atoms': [{'elements': ['C'], 'charge': 0, 'ring': False, 'aromatic': False}, {}], 'bonds': [{'a': 0, 'b': 1}]},
]


def corpus_targets():
    """(targets, names) of the frozen corpus of molkey_reference.corpus(); the Kekulé properties are left out (no pattern of PATTERNS
    reads them)."""
    mols, _, _, names = Q.corpus()
    return [target_of_mol(m, kekule=False) for m in mols], names


# ---- comparing an implementation's row with the restatement's ---------------------------------------------------------------------------
def check_row(got, want, target, p, where=''):
    """got: {'embeddings', 'anchors', 'mask' (int), 'first' (16 ints), 'status'} of the code under test for one (graph, pattern);
    want: `search`'s dict for the same max_steps.  SUB_TRUNCATED must agree; an untruncated row must be equal, a truncated one within
    what the definition promises."""
    assert bool(got['status'] & S.SUB_TRUNCATED) == want['truncated'], (where, got, want['steps'])
    if not want['truncated']:
        mine = {k: want[k] for k in ('embeddings', 'anchors', 'mask', 'first', 'status')}
        assert got == mine, (where, got, mine)
        return
    assert 0 <= got['embeddings'] <= want['embeddings'] and 0 <= got['anchors'] <= want['anchors'], (where, got)
    assert got['mask'] & ~want['mask'] == 0, (where, got)
    k = len(p['atoms'])
    first = list(got['first'])
    assert first[k:] == [-1] * (S.MAX_ATOMS - k), (where, got)
    if first[0] >= 0:
        assert is_embedding(target, p, first[:k]), (where, got)
    else:
        assert first == [-1] * S.MAX_ATOMS, (where, got)
    assert bool(got['status'] & S.SUB_OUT_OF_BOUNDS) == want['bounded'] and not got['status'] & S.SUB_NO_KEKULE, (where, got)
    assert bool(got['status'] & S.SUB_MATCHED) == (got['embeddings'] > 0), (where, got)


# ---- the host program (tools/mol_sub_host_check.cpp) ------------------------------------------------------------------------------
def write_host_cases(path, cases):
    """cases: [(target, pattern table row as 416 ints, max_steps)] in the program's text form."""
    with open(path, 'w') as fh:
        fh.write('%d\n' % len(cases))
        for target, row, max_steps in cases:
            pairs = sorted((a, b) for (a, b) in target['bonds'] if a < b)
            fh.write('%d %d %d %d\n' % (len(target['atoms']), len(pairs), max_steps, int(target['kekule_failed'])))
            for a in target['atoms']:
                fh.write('%d %d %d %d\n' % (a['cls'], a['hcount'], a['charge'], int(a['ring'])))
            for a, b in pairs:
                fh.write('%d %d %d %d\n' % (a, b, target['bonds'][(a, b)][0], int(target['bonds'][(a, b)][1])))
            fh.write(' '.join(str(int(v)) for v in row) + '\n')


def read_host_answers(text):
    """[(check code, row dict in `check_row`'s form)] of the program's output."""
    out = []
    for line in text.strip().split('\n'):
        v = [int(x) for x in line.split()]
        out.append((v[0], {'embeddings': v[1], 'anchors': v[2], 'mask': v[3] | v[4] << 64, 'status': v[5], 'first': v[6:6 + S.MAX_ATOMS]}))
    return out
