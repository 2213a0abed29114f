"""Plain restatement of the stereo perception and of the isomeric SMILES (DESIGN.md 2.9 "Stereo"; phoregen_amd/molecule.py,
csrc/mol_stereo.hip, csrc/mol_smiles.hip) for the tests, and an independent reader of the isomeric text.

The perception is float64 over numpy vectors and Python ints masked to 64 bits; the colours and the key come from
tests/molkey_reference.py.  The writer is recursive over dicts, as tests/smiles_reference.py's, and settles the '/' and '\\' marks with
a union-find with parities instead of the kernel's breadth-first walk.  The reader parses the text by the OpenSMILES definition alone
-- the order in which a chiral atom's neighbours stand in the text, '@' = counter-clockwise seen from the first, '/' and '\\' as
"above" and "below" an end of a double bond -- and knows nothing of the writer's rules; `check_text_against_geometry` holds what it
reads against the coordinates.  Also here: `all_rows`, which gathers everything the kernels read for one graph from the other
restatements (tests/hydrogen_reference.py uses it too), the generator of the size family, the hand examples with their coordinates,
and the case format of tools/stereo_host_check.cpp.  Nothing here holds device code."""
import math
import os
import sys

import numpy as np
import torch

import kekule_reference as K
import mol_support as MS
import molkey_reference as KEY
import ring_reference as G
import smiles_reference as S
from mol_support import C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, M64, batch_from, mirrored  # noqa: F401  (read from here by the tests)
from phoregen_amd import molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

UNDEF = M.STEREO_UNDEFINED_VALUE
CENTRE_CLASSES = tuple(ATOM_TYPES.index(z) for z in M.STEREO_CENTRE_CLASSES)
MARGIN = 1e-4                    # no generated |V| or |t| lies closer than this to its threshold; fp32 moves either by about 1e-6


def perm_sign(seq):
    """The sign of the permutation that sorts `seq` (distinct, comparable): by its cycles."""
    want = sorted(seq)
    to = [want.index(x) for x in seq]
    seen, sign = [False] * len(to), 1
    for i in range(len(to)):
        if not seen[i]:
            k, length = i, 0
            while not seen[k]:
                seen[k], k, length = True, to[k], length + 1
            sign *= -1 if length % 2 == 0 else 1
    return sign


# ---- section 1: perception ----------------------------------------------------------------------------------------------------------------
def graph_of_rows(cls, order):
    """kept [n], nbrs [n] (ascending) and the bond rows {(a, b): row} of a graph as the ring screen reads it."""
    return MS.pair_walk(cls, order)[:3]


def _unit(c, p):
    d = p - c
    length = math.sqrt(float(d @ d))
    return None if not math.isfinite(length) or length == 0.0 else d / length


def centre_volume(pos, c, nbrs):
    """V of the centre c with the neighbours `nbrs` in the order given (three: the fourth ligand is the hydrogen); None if a vector has
    no length or is not finite."""
    u = [_unit(pos[c], pos[k]) for k in nbrs]
    if any(x is None for x in u):
        return None
    if len(u) == 3:
        u.append(-(u[0] + u[1] + u[2]))
    v = float((u[0] - u[3]) @ np.cross(u[1] - u[3], u[2] - u[3]))
    return v if math.isfinite(v) else None


def bond_planarity(pos, a, b, ra, rb):
    """t of the double bond a - b with the substituents ra of a and rb of b; None if it has no value."""
    e, da, db = pos[b] - pos[a], pos[ra] - pos[a], pos[rb] - pos[b]
    ee, la, lb = float(e @ e), math.sqrt(float(da @ da)), math.sqrt(float(db @ db))
    if not all(math.isfinite(x) for x in (ee, la, lb)) or ee == 0.0 or la == 0.0 or lb == 0.0:
        return None
    wa, wb = da - e * float(da @ e) / ee, db - e * float(db @ e) / ee
    t = float(wa @ wb) / (la * lb)
    return t if math.isfinite(t) else None


def stereo_of_rows(cls, order, kekule_order, hcount, kekule_status, ring_size, colour, key, pos, limits=None):
    """Section 1 for one graph as the device holds it.  colour: unsigned ints [n], key: unsigned int, pos [n, 3].  Returns the kernel's
    outputs -- 'atom_parity', 'atom_label' int8 [n], 'bond_stereo', 'bond_label' int8 [h], 'stereo_key' (unsigned int), 'counts' int32
    [8], 'status', 'ok' -- and 'volumes' {atom: V} / 'planarities' {row: t} of the stereogenic elements (None: no value)."""
    limits = M.StereoLimits() if limits is None else limits
    n, h = len(cls), len(order)
    out = {'atom_parity': np.zeros(n, dtype=np.int8), 'atom_label': np.zeros(n, dtype=np.int8), 'bond_stereo': np.zeros(h, dtype=np.int8),
           'bond_label': np.zeros(h, dtype=np.int8), 'stereo_key': int(key) & M64, 'counts': np.zeros(8, dtype=np.int32), 'volumes': {},
           'planarities': {}}
    if int(kekule_status) & M.KEKULE_FAILED:
        return dict(out, status=M.STEREO_NO_KEKULE, ok=False)
    pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
    colour = [int(c) & M64 for c in colour]
    kek, hc = [int(o) for o in kekule_order], [int(x) for x in hcount]
    kept, nbrs, rows = graph_of_rows(cls, order)
    counts = dict.fromkeys(M.STEREO_COUNTS, 0)
    total = 0
    # centres
    for c in range(n):
        deg = len(nbrs[c])
        if not (kept[c] and int(cls[c]) in CENTRE_CLASSES and ((deg == 4 and hc[c] == 0) or (deg == 3 and hc[c] == 1))):
            continue
        counts['centre_candidates'] += 1
        cols = [colour[k] for k in nbrs[c]]
        if len(set(cols)) != deg:
            continue
        counts['centres_stereogenic'] += 1
        v = out['volumes'][c] = centre_volume(pos, c, nbrs[c])
        if v is None or abs(v) < limits.vol_min:
            out['atom_parity'][c] = out['atom_label'][c] = UNDEF
            counts['centres_undefined'] += 1
            continue
        parity = 1 if v > 0 else -1
        label = parity * perm_sign(cols)                               # (the hydrogen is last before and after the sort)
        out['atom_parity'][c], out['atom_label'][c] = parity, label
        counts['centres_defined'] += 1
        total = (total + KEY.mix(colour[c] ^ (M.STEREO_KEY_A if label > 0 else M.STEREO_KEY_B))) & M64
    # double bonds
    multi = [sum(kek[rows[(min(x, k), max(x, k))]] >= 2 for k in nbrs[x]) for x in range(n)]
    for (a, b), row in rows.items():
        if not (kek[row] == 2 and int(order[row]) != 4 and int(ring_size[row]) == 0):
            continue
        if not all(multi[x] == 1 and (len(nbrs[x]) == 3 or (len(nbrs[x]) == 2 and hc[x] <= 1)) for x in (a, b)):
            continue
        counts['bond_candidates'] += 1
        subs = {a: [k for k in nbrs[a] if k != b], b: [k for k in nbrs[b] if k != a]}
        if any(len(s) == 2 and colour[s[0]] == colour[s[1]] for s in subs.values()):
            continue
        counts['bonds_stereogenic'] += 1
        t = out['planarities'][row] = bond_planarity(pos, a, b, subs[a][0], subs[b][0])
        if t is None or abs(t) < limits.planar_min:
            out['bond_stereo'][row] = out['bond_label'][row] = UNDEF
            counts['bonds_undefined'] += 1
            continue
        stereo = label = 1 if t > 0 else -1
        for x in (a, b):
            # the substituents by ascending colour, the hydrogen last: is the largest one the lowest-index one?
            ranked = sorted(subs[x], key=lambda k: colour[k]) + (['H'] if len(subs[x]) == 1 and hc[x] >= 1 else [])
            if ranked[-1] != subs[x][0]:
                label = -label
        out['bond_stereo'][row], out['bond_label'][row] = stereo, label
        counts['bonds_defined'] += 1
        word = (KEY.mix(colour[a]) + KEY.mix(colour[b])) & M64
        total = (total + KEY.mix(word ^ (M.STEREO_KEY_C if label > 0 else M.STEREO_KEY_D))) & M64
    if counts['centres_defined'] + counts['bonds_defined'] > 0:
        out['stereo_key'] = KEY.mix((int(key) & M64) ^ KEY.mix(total))
    status = 0
    status |= M.STEREO_UNDEFINED if counts['centres_undefined'] + counts['bonds_undefined'] > limits.max_undefined else 0
    status |= M.STEREO_HAS_CENTRE if counts['centres_defined'] else 0
    status |= M.STEREO_HAS_BOND if counts['bonds_defined'] else 0
    status |= M.STEREO_NONFINITE if any(kept[i] and not np.isfinite(pos[i]).all() for i in range(n)) else 0
    out['counts'] = np.array([counts[k] for k in M.STEREO_COUNTS], dtype=np.int32)
    return dict(out, status=status, ok=status & M.STEREO_FAIL_MASK == 0)


def numbering_proof(rows, limits=None):
    """Does no renumbering of the atoms move an answer of this graph (an `all_rows` record)?  A centre's |V| is the same for every order
    of its neighbours, but a double bond is judged on its LOWEST-INDEX substituents: on a distorted geometry another pair of
    substituents can give another |t|, on the other side of planar_min, or a sign that does not go with it.  True iff, for every
    stereogenic double bond, all choices of substituents give |t| >= planar_min + MARGIN with the signs of a planar bond, or all give
    |t| < planar_min - MARGIN; and no |V| lies within MARGIN of vol_min."""
    limits = M.StereoLimits() if limits is None else limits
    r, pos = restate(rows, limits), rows.pos
    if any(v is None or abs(abs(v) - limits.vol_min) <= MARGIN for v in r['volumes'].values()):
        return False
    _, nbrs, at = graph_of_rows(rows.cls, rows.order)
    for (a, b), row in at.items():
        if r['bond_stereo'][row] == 0:
            continue
        sa, sb = [k for k in nbrs[a] if k != b], [k for k in nbrs[b] if k != a]
        ts = {(i, j): bond_planarity(pos, a, b, x, y) for i, x in enumerate(sa) for j, y in enumerate(sb)}
        if any(t is None for t in ts.values()):
            return False
        if all(abs(t) < limits.planar_min - MARGIN for t in ts.values()):
            continue
        if not all(abs(t) >= limits.planar_min + MARGIN and (t > 0) == ((ts[(0, 0)] > 0) == ((i + j) % 2 == 0)) for (i, j), t in ts.items()):
            return False
    return True


def all_rows(classes, bonds, pos, allow_charged=True, with_keys_and_rings=True):
    """Everything the kernels read for one (classes, {(a, b): bond class}, coordinates) graph, by the other restatements, as a
    `mol_support.MolRows`: the rows, the Kekulé form, pos as the float64 of its fp32 rounding and, with_keys_and_rings, the ring
    sizes, the colours and the key (None without)."""
    cls, order = MS.rows_of(classes, bonds)
    k = K.kekule_of_rows(cls, order, allow_charged)
    key, colour = KEY.key_of_rows(cls, order) if with_keys_and_rings else (None, None)
    return MS.MolRows(cls, order, k['kekule_order'], k['hcount'], k['charge'], int(k['status']),
                      G.rings_of_rows(cls, order)['ring_size'] if with_keys_and_rings else None, colour, key,
                      np.asarray(pos, dtype=np.float32).astype(np.float64).reshape(len(classes), 3))


def restate(rows, limits=None):
    """`stereo_of_rows` on an `all_rows` record."""
    return stereo_of_rows(rows.cls, rows.order, rows.kekule_order, rows.hcount, rows.kekule_status, rows.ring_size, rows.colour, rows.key,
                          rows.pos, limits)


def stereo_of(classes, bonds, pos, limits=None):
    return restate(all_rows(classes, bonds, pos), limits)


def same_stereo(got, want, where=''):
    """Every output `==`."""
    for k in ('atom_parity', 'atom_label', 'bond_stereo', 'bond_label', 'counts'):
        assert np.asarray(got[k]).tolist() == np.asarray(want[k]).tolist(), (where, k, np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())
    assert int(got['stereo_key']) & M64 == want['stereo_key'], (where, 'stereo_key')
    assert int(got['status']) == want['status'], (where, 'status', got['status'], want['status'])


# ---- section 2: the writer ----------------------------------------------------------------------------------------------------------------
class _Parity:
    """Union-find over the marked bonds with the parity of every bond relative to its root."""

    def __init__(self):
        self.up, self.rel, self.bad = {}, {}, set()

    def find(self, x):
        self.up.setdefault(x, x), self.rel.setdefault(x, 1)
        if self.up[x] == x:
            return x, 1
        root, r = self.find(self.up[x])
        self.up[x], self.rel[x] = root, self.rel[x] * r
        return root, self.rel[x]

    def relate(self, x, y, product):
        """mark(x) * mark(y) = product"""
        (rx, px), (ry, py) = self.find(x), self.find(y)
        if rx == ry:
            if px * py != product:
                self.bad.add(rx)
            return
        self.up[rx], self.rel[rx] = ry, px * py * product
        if rx in self.bad:
            self.bad.discard(rx), self.bad.add(ry)


def write_graph(elements, bonds, hcount, charge, parity, stereo):
    """Section 2 for one graph given as dicts over the kept atoms' local indices: elements {i: z}, bonds {(a, b): 1 | 2 | 3} with a < b,
    hcount, charge, parity {i: value}, stereo {(a, b): value}.  Returns `smiles_reference.write_graph`'s dict plus 'centres',
    'clockwise', 'marked', 'expressed', 'dropped'; raises smiles_reference.RingLabels."""
    nbr = {i: {} for i in elements}
    for (a, b), o in bonds.items():
        nbr[a][b] = nbr[b][a] = o
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    rank, parent, children = {}, {}, {i: [] for i in elements}

    def walk(v):
        rank[v] = len(rank)
        for w in sorted(nbr[v]):
            if w not in rank:
                parent[w] = v
                children[v].append(w)
                walk(w)

    roots = []
    for i in sorted(elements):
        if i not in rank:
            roots.append(i)
            parent[i] = None
            walk(i)
    opens, closes = {i: [] for i in elements}, {i: [] for i in elements}
    for (a, b) in bonds:
        if parent[a] != b and parent[b] != a:
            anc, desc = (a, b) if rank[a] < rank[b] else (b, a)
            opens[anc].append(desc)
            closes[desc].append(anc)
    # ---- the double bonds the text can express, and the marks of the single bonds next to them ----
    def subs_of(x, y):
        return sorted(k for k in nbr[x] if k != y)

    def end_ok(x, y):
        return len(subs_of(x, y)) in (1, 2) and all(nbr[x][k] == 1 for k in subs_of(x, y))

    doubles = [(a, b, int(s)) for (a, b), s in sorted(stereo.items())
               if int(s) in (1, -1) and bonds.get((a, b)) == 2 and end_ok(a, b) and end_ok(b, a)]
    first = lambda x, r: 1 if rank[x] < rank[r] else -1                # noqa: E731  (x is written before r)
    pair = lambda x, r: (min(x, r), max(x, r))                         # noqa: E731
    uf = _Parity()
    for a, b, s in doubles:
        ra, rb = subs_of(a, b), subs_of(b, a)
        uf.relate(pair(a, ra[0]), pair(b, rb[0]), s * first(a, ra[0]) * first(b, rb[0]))
        for x, r in ((a, ra), (b, rb)):
            if len(r) == 2:
                uf.relate(pair(x, r[0]), pair(x, r[1]), -first(x, r[0]) * first(x, r[1]))

    def place(p):                                                      # where the bond's symbol stands in the text
        x, y = (p[0], p[1]) if rank[p[0]] < rank[p[1]] else (p[1], p[0])
        return (rank[y], 0, 0) if parent[y] == x else (rank[x], 1, y)

    groups = {}
    for p in list(uf.up):
        groups.setdefault(uf.find(p)[0], []).append(p)
    mark = {}
    for root, members in groups.items():
        if root in uf.bad:
            continue
        lead = min(members, key=place)
        for p in members:
            mark[p] = uf.find(p)[1] * uf.find(lead)[1]                 # the first in the text is '/'
    expressed = sum(1 for a, b, _ in doubles if pair(a, subs_of(a, b)[0]) in mark)
    in_use, label = set(), {}
    stats = {'max_label': 0, 'bracket_atoms': 0, 'branches': 0, 'centres': 0, 'clockwise': 0}

    def symbol(x, y):
        p = pair(x, y)
        return {1: '/', -1: '\\'}[mark[p]] if p in mark else S.BOND_SYMBOL[nbr[x][y]]

    def token(v):
        z, h, q, par = elements[v], hcount[v], charge[v], int(parity.get(v, 0))
        if par in (1, -1) and ((len(nbr[v]) == 4 and h == 0) or (len(nbr[v]) == 3 and h == 1)):
            index_order = sorted(nbr[v]) + (['H'] if h == 1 else [])
            text_order = ([parent[v]] if parent[v] is not None else []) + (['H'] if h == 1 else []) + sorted(closes[v]) + sorted(opens[v]) \
                + children[v]
            sign = perm_sign([text_order.index(x) for x in index_order])
            stats['centres'] += 1
            stats['clockwise'] += par * sign < 0
            return '[' + M.ELEMENT_SYMBOL[z] + ('@' if par * sign > 0 else '@@') + ('H' if h == 1 else '') + ('+' if q == 1 else '') + ']', True
        return S.atom_token(z, sum(nbr[v].values()), h, q)

    def visit(v):
        tok, bracket = token(v)
        stats['bracket_atoms'] += bracket
        text = (symbol(parent[v], v) if parent[v] is not None else '') + tok
        for a in sorted(closes[v]):
            text += S.label_text(label[(a, v)])
        for d in sorted(opens[v]):
            free = [k for k in range(1, M.SMILES_MAX_LABEL + 1) if k not in in_use]
            if not free:
                raise S.RingLabels()
            label[(v, d)] = free[0]
            in_use.add(free[0])
            stats['max_label'] = max(stats['max_label'], free[0])
            text += symbol(v, d) + S.label_text(free[0])
        for a in closes[v]:
            in_use.discard(label[(a, v)])
        for c in children[v][:-1]:
            stats['branches'] += 1
            text += '(' + visit(c) + ')'
        if children[v]:
            text += visit(children[v][-1])
        return text

    text = '.'.join(visit(r) for r in roots)
    return dict(stats, text=text, rank=rank, components=len(roots), ring_closures=sum(len(v) for v in opens.values()), marked=len(mark),
                expressed=expressed, dropped=len(uf.bad))


def smiles_of_rows(cls, kekule_order, hcount, charge, kekule_status, atom_parity, bond_stereo, capacity=None):
    """The restatement's answer for one graph as the device holds it, in `smiles_reference.smiles_of_rows`' form plus 'stereo_counts'
    (int32 [4]); capacity None = 12 * max(n, 8)."""
    cls, kek = [int(c) for c in cls], [int(o) for o in kekule_order]
    n = len(cls)
    capacity = 12 * max(n, 8) if capacity is None else capacity
    failed = lambda bit: {'text': '', 'status': bit, 'ok': False, 'length': 0, 'counts': np.zeros(8, dtype=np.int32),   # noqa: E731
                          'atom_rank': np.full(n, -1, dtype=np.int16), 'stereo_counts': np.zeros(4, dtype=np.int32)}
    if kekule_status & M.KEKULE_FAILED:
        return failed(M.SMILES_NO_KEKULE)
    elements = {i: ATOM_TYPES[c] for i, c in enumerate(cls) if 0 <= c <= 10}
    at = MS.pair_walk(cls, kek, (1, 2, 3)).rows
    bonds, stereo = {p: kek[row] for p, row in at.items()}, {p: int(bond_stereo[row]) for p, row in at.items()}
    try:
        w = write_graph(elements, bonds, {i: int(hcount[i]) for i in elements}, {i: int(charge[i]) for i in elements},
                        {i: int(atom_parity[i]) for i in elements}, stereo)
    except S.RingLabels:
        return failed(M.SMILES_RING_LABELS)
    text = w['text']
    fits = len(text) <= capacity
    status = (0 if fits else M.SMILES_TOO_LONG) | (M.SMILES_DISCONNECTED if '.' in text else 0) | (0 if elements else M.SMILES_EMPTY)
    status |= (M.SMILES_BRACKET if w['bracket_atoms'] else 0) | (M.SMILES_STEREO_DROPPED if w['dropped'] else 0)
    counts = {'length': len(text), 'atoms': len(elements), 'bonds': len(bonds), 'components': w['components'],
              'ring_closures': w['ring_closures'], 'branches': w['branches'], 'max_label': w['max_label'], 'bracket_atoms': w['bracket_atoms']}
    return {'text': text if fits else '', 'status': status, 'ok': fits, 'length': len(text) if fits else 0,
            'counts': np.array([counts[k] for k in M.SMILES_COUNTS], dtype=np.int32),
            'atom_rank': np.array([w['rank'][i] if fits and i in elements else -1 for i in range(n)], dtype=np.int16),
            'stereo_counts': np.array([w['centres'], w['clockwise'], w['marked'], w['expressed']], dtype=np.int32)}


def same_text(got, want, where=''):
    S.same_answer(got, want, where)
    assert np.asarray(got['stereo_counts']).tolist() == want['stereo_counts'].tolist(), (where, got['stereo_counts'], want['stereo_counts'])


# ---- the independent reader ---------------------------------------------------------------------------------------------------------------
_Z = {sym: z for z, sym in M.ELEMENT_SYMBOL.items()}
_SYMBOLS = sorted(_Z, key=len, reverse=True)
_BOND = {'=': 2, '#': 3, '/': 1, '\\': 1}


def read_isomeric(text):
    """Parse isomeric OpenSMILES as far as the writer's alphabet goes.  Returns (atoms, bonds, centres, sides):
    atoms [(z, hydrogens or None for a bare atom, charge)] in text order; bonds {(i, j): order}, i < j;
    centres {i: ('@' | '@@', [its neighbours in the order OpenSMILES defines: the atom before it, its implicit hydrogen 'H', its
    ring-closure digits as they stand, its branches and its successor])};
    sides {(x, r): +1 | -1}: seen from x, an end of some double bond, the single bond to r points "up" (+1) or "down" (-1) -- `a/b`
    is up from a and down from b."""
    atoms, bonds, centres, sides = [], {}, {}, {}
    order_of = []                                                      # per atom: its neighbours as the text gives them
    stack, prev, pending, rings = [], None, None, {}
    k = 0

    def direction(x, y, sym):                                          # the symbol stands between x (first) and y
        if sym in ('/', '\\'):
            up = 1 if sym == '/' else -1
            for key, val in (((x, y), up), ((y, x), -up)):
                if sides.setdefault(key, val) != val:
                    raise ValueError('%r: two directions on one bond' % text)

    def join(i, j, sym):
        key = (min(i, j), max(i, j))
        if i == j or key in bonds:
            raise ValueError('%r: second bond or self bond' % text)
        bonds[key] = _BOND.get(sym, 1)

    while k < len(text):
        ch = text[k]
        if ch == '[' or ch.isalpha():
            chir, h, q = None, None, 0
            if ch == '[':
                end = text.index(']', k)
                body = text[k + 1:end]
                k = end + 1
                sym = next((s for s in _SYMBOLS if body.startswith(s)), None)
                if sym is None:
                    raise ValueError('%r: atom %r' % (text, body))
                rest, h = body[len(sym):], 0
                if rest.startswith('@'):
                    chir, rest = ('@@', rest[2:]) if rest.startswith('@@') else ('@', rest[1:])
                if rest.startswith('H'):
                    digits = ''.join(c for c in rest[1:] if c.isdigit())
                    h, rest = int(digits) if digits else 1, rest[1 + len(digits):]
                if rest.startswith('+'):
                    q, rest = 1, rest[1:]
                if rest:
                    raise ValueError('%r: atom %r' % (text, body))
            else:
                sym = next((s for s in _SYMBOLS if text.startswith(s, k)), None)
                if sym is None:
                    raise ValueError('%r: %r at %d' % (text, ch, k))
                k += len(sym)
            me = len(atoms)
            atoms.append((_Z[sym], h, q))
            order_of.append([])
            if prev is not None:
                join(prev, me, pending)
                direction(prev, me, pending or '')
                order_of[prev].append(me)
                order_of[me].append(prev)
            elif pending is not None:
                raise ValueError('%r: bond symbol without an atom before it' % text)
            if chir:
                if h not in (0, 1):
                    raise ValueError('%r: a chiral atom with %d hydrogens' % (text, h))
                centres[me] = chir
                if h == 1:
                    order_of[me].append('H')
            prev, pending = me, None
        elif ch in _BOND:
            if pending is not None or prev is None:
                raise ValueError('%r: bond symbol at %d' % (text, k))
            pending, k = ch, k + 1
        elif ch == '(':
            if prev is None or pending is not None:
                raise ValueError('%r: ( at %d' % (text, k))
            stack.append(prev)
            k += 1
        elif ch == ')':
            if not stack or pending is not None:
                raise ValueError('%r: ) at %d' % (text, k))
            prev, k = stack.pop(), k + 1
        elif ch == '.':
            if stack or pending is not None or prev is None:
                raise ValueError('%r: . at %d' % (text, k))
            prev, k = None, k + 1
        elif ch.isdigit() or ch == '%':
            lab, k = (int(text[k + 1:k + 3]), k + 3) if ch == '%' else (int(ch), k + 1)
            if prev is None:
                raise ValueError('%r: label without an atom' % text)
            if lab in rings:
                other, sym, slot = rings.pop(lab)
                if sym is not None and pending is not None and _BOND[sym] != _BOND[pending]:
                    raise ValueError('%r: label %d with two bond orders' % (text, lab))
                join(other, prev, pending or sym)
                direction(other, prev, sym or '')                      # a symbol at the opening digit reads from the opener
                direction(prev, other, pending or '')                  # ... at the closing digit from the closer
                order_of[other][slot] = prev
                order_of[prev].append(other)
            else:
                rings[lab] = (prev, pending, len(order_of[prev]))
                order_of[prev].append(None)
            pending = None
        else:
            raise ValueError('%r: %r at %d' % (text, ch, k))
    if stack or rings or pending is not None:
        raise ValueError('%r: unclosed branch, ring or bond' % text)
    return atoms, bonds, {i: (c, order_of[i]) for i, c in centres.items()}, sides


def plain_text(text):
    """The text without its stereo: marks taken out, a chiral bracket atom without its '@'s."""
    return text.replace('/', '').replace('\\', '').replace('@', '')


def check_text_against_geometry(text, atom_rank, pos, want, rows, limits=None, where=''):
    """What the reader derives from the text, held against the coordinates in float64: every centre the text marks has the
    handedness it says (OpenSMILES: seen from its first neighbour the others run counter-clockwise for '@'), every double bond of
    `want` that is cis or trans reads as that, and the text marks exactly the centres and expresses at least the double bonds that
    `want` (a `stereo_of_rows` result) has as +1 / -1.  atom_rank: the writer's; rows: {(a, b): pair row}.  Returns (centres, double
    bonds read, double bonds the text fixes beyond those of `want`)."""
    limits = M.StereoLimits() if limits is None else limits
    atoms, bonds, centres, sides = read_isomeric(text)
    at = {int(r): i for i, r in enumerate(atom_rank) if r >= 0}        # text position -> local index
    pos = np.asarray(pos, dtype=np.float64)
    assert sorted(at[i] for i in centres) == [i for i in range(len(atom_rank)) if want['atom_parity'][i] in (1, -1)], (where, text)
    for i, (chir, around) in centres.items():
        assert len(around) == 4 and len(set(map(str, around))) == 4, (where, text, around)
        heavy = [at[x] for x in around if x != 'H']
        u = [_unit(pos[at[i]], pos[x]) for x in heavy]
        if len(heavy) == 3:
            u.insert(around.index('H'), -(u[0] + u[1] + u[2]))
        v = float((u[0] - u[3]) @ np.cross(u[1] - u[3], u[2] - u[3]))   # > 0: from u[0], the others run counter-clockwise
        assert abs(v) >= limits.vol_min - MARGIN and (v > 0) == (chir == '@'), (where, text, i, chir, v)
    read, extra = 0, 0
    for (i, j), o in bonds.items():
        if o != 2:
            continue
        ends = []
        for x, y in ((i, j), (j, i)):
            seen = {r: s for (e, r), s in sides.items() if e == x and r != y}
            if len(seen) == 2 and len(set(seen.values())) != 2:
                raise AssertionError((where, text, 'both substituents of %d on one side' % x))
            ends.append(seen)
        a, b = sorted((at[i], at[j]))
        stereo = int(want['bond_stereo'][rows[(a, b)]])
        if not ends[0] or not ends[1]:
            assert stereo not in (1, -1), (where, text, (a, b), 'not expressed')
            continue
        # the side of the lowest-index substituent of either end, from whichever substituent the text gives a side
        says = 1
        for x, seen in zip((i, j), ends):
            other = j if x == i else i
            subs = sorted((q if p == x else p for (p, q) in bonds if x in (p, q) and other not in (p, q)), key=lambda r: at[r])
            says *= seen[subs[0]] if subs[0] in seen else -next(iter(seen.values()))
        if stereo in (1, -1):
            assert says == stereo, (where, text, (a, b), says, stereo)
            read += 1
        else:
            extra += 1
    return len(centres), read, extra


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
FAMILY_SIZES = (1, 2, 4, 5, 9, 10, 63, 64, 65, 127, 128)
FAMILY_SEED = 20250314
FAMILY_GRAPHS = 66
CENTRE_AT = (0, 63, 64, 127)
NEIGHBOURS_AT = (62, 63, 64, 65)


def random_graph(rng, n):
    """A tree of n atoms with degree at most 4, a few ring closures, mostly carbon, some double bonds apart from each other."""
    classes = [int(v) for v in rng.choice([C_] * 8 + [N_, N_, O_, F_, CL_, BR_, S_, P_, SI_], n)]
    bonds, degree, multi = {}, [0] * n, [False] * n
    for v in range(1, n):
        u = int(rng.integers(max(0, v - 5), v))
        for _ in range(64):
            if degree[u] < (4 if classes[u] in (C_, N_, SI_, P_, S_) else 2):
                break
            u = int(rng.integers(0, v))
        double = rng.random() < 0.3 and not multi[u] and classes[u] in (C_, N_) and classes[v] in (C_, N_) and degree[u] < 3
        bonds[(u, v)] = 2 if double else 1
        multi[u], multi[v] = multi[u] or double, multi[v] or double
        degree[u] += 1
        degree[v] += 1
    for _ in range(int(rng.integers(0, 3)) if n > 6 else 0):
        a, b = sorted(int(v) for v in rng.choice(n, 2, replace=False))
        if (a, b) not in bonds and degree[a] < 3 and degree[b] < 3:
            bonds[(a, b)] = 1
            degree[a] += 1
            degree[b] += 1
    return classes, bonds


def renumbered(classes, bonds, pos, perm):
    """The same graph with atom i renumbered to perm[i]."""
    cl, bo = KEY.permuted(classes, bonds, perm)
    out = np.empty_like(pos)
    out[np.asarray(perm)] = pos
    return cl, bo, out


def _placed(rng, classes, bonds, k):
    """The graph renumbered so that a centre candidate sits at one of CENTRE_AT (graph k takes the k-th), or so that the neighbours of
    a candidate with four are NEIGHBOURS_AT; unchanged if it has none that fits."""
    n = len(classes)
    nbrs = [[] for _ in range(n)]
    for a, b in bonds:
        nbrs[a].append(b), nbrs[b].append(a)
    cands = [i for i in range(n) if classes[i] in CENTRE_CLASSES and len(nbrs[i]) in (3, 4)]
    perm = list(range(n))

    def swap(i, j):                                                    # atom i goes to place j, whatever sat there takes i's
        x = perm.index(j)
        perm[i], perm[x] = perm[x], perm[i]

    four = [i for i in cands if len(nbrs[i]) == 4]
    if k % 5 == 4 and four and n > max(NEIGHBOURS_AT) + 1:
        c = four[0]
        for x, place in zip(nbrs[c], NEIGHBOURS_AT):
            swap(x, place)
        if perm[c] in NEIGHBOURS_AT:
            return classes, bonds
    elif cands and CENTRE_AT[k % 4] < n:
        swap(cands[int(rng.integers(0, len(cands)))], CENTRE_AT[k % 4])
    else:
        return classes, bonds
    return KEY.permuted(classes, bonds, perm)


def family(seed=FAMILY_SEED, n_graphs=FAMILY_GRAPHS, sizes=FAMILY_SIZES, limits=None):
    """[(classes, bonds, pos float32 [n, 3])]: the sizes in turn, coordinates drawn at random (perception needs no sensible geometry)
    and drawn again, by the restatement alone, until no stereogenic |V| lies within MARGIN of vol_min and no |t| within MARGIN of
    planar_min; plus two graphs without a Kekulé structure."""
    limits = M.StereoLimits() if limits is None else limits
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_graphs):
        n = sizes[k % len(sizes)]
        classes, bonds = _placed(rng, *random_graph(rng, n), k // len(sizes))
        if k >= n_graphs - 2:
            classes, bonds = K.NAMED['all-carbon five-ring'][:2]
        for _ in range(100):
            pos = (rng.normal(size=(len(classes), 3)) * 1.5).astype(np.float32)
            r = stereo_of(classes, bonds, pos, limits)
            if (all(v is not None and abs(abs(v) - limits.vol_min) > MARGIN for v in r['volumes'].values())
                    and all(t is not None and abs(abs(t) - limits.planar_min) > MARGIN for t in r['planarities'].values())):
                break
        else:
            raise AssertionError('no coordinates clear of the thresholds')
        out.append((list(classes), dict(bonds), pos))
    return out


def census(graphs, limits=None):
    """What the restatement finds in `graphs`, before any kernel output exists."""
    c = dict.fromkeys(('centres+', 'centres-', 'centres_undefined', 'centres_h', 'cis', 'trans', 'bonds_undefined', 'no_kekule'), 0)
    at, around = set(), False
    for classes, bonds, pos in graphs:
        r = stereo_of(classes, bonds, pos, limits)
        _, nbrs, _ = graph_of_rows(*MS.rows_of(classes, bonds))
        c['no_kekule'] += r['status'] == M.STEREO_NO_KEKULE
        for i, p in enumerate(r['atom_parity'].tolist()):
            c['centres+'] += p == 1
            c['centres-'] += p == -1
            c['centres_undefined'] += p == UNDEF
            c['centres_h'] += p != 0 and len(nbrs[i]) == 3
            if p != 0:
                at.add(i)
                around = around or tuple(nbrs[i]) == NEIGHBOURS_AT
        for s in r['bond_stereo'].tolist():
            c['cis'] += s == 1
            c['trans'] += s == -1
            c['bonds_undefined'] += s == UNDEF
    return c, at, around


# ---- the hand examples: name: (classes, bonds, coordinates in Angstrom, isomeric text) -------------------------------------------------------
# The first three sets of coordinates were written by hand (a tetrahedron's corners; a planar sp2 skeleton), the others come from a
# distance-geometry embedding of ideal bond lengths and angles, rounded to three decimals.  The texts were checked by hand against the
# coordinates: `check_text_against_geometry` repeats that check for every one of them.
_TARTARIC = ([C_, O_, O_, C_, O_, C_, O_, C_, O_, O_],
             {(0, 1): 2, (0, 2): 1, (0, 3): 1, (3, 4): 1, (3, 5): 1, (5, 6): 1, (5, 7): 1, (7, 8): 2, (7, 9): 1})
_DIFLUORO = ([F_, C_, C_, F_], {(0, 1): 1, (1, 2): 2, (2, 3): 1})
EXAMPLES = {
    'CHFClBr skeleton': ([C_, F_, CL_, BR_], {(0, 1): 1, (0, 2): 1, (0, 3): 1},
                         [[0.0, 0.0, 0.0], [-0.8, 0.8, 0.8], [-1.0, -1.0, -1.0], [1.1, 1.1, -1.1]], '[C@H](F)(Cl)Br'),
    'cis-1,2-difluoroethene skeleton': (*_DIFLUORO, [[-0.67, 1.16, 0.0], [0.0, 0.0, 0.0], [1.33, 0.0, 0.0], [2.0, 1.16, 0.0]], 'F/C=C\\F'),
    'trans-1,2-difluoroethene skeleton': (*_DIFLUORO, [[-0.67, 1.16, 0.0], [0.0, 0.0, 0.0], [1.33, 0.0, 0.0], [2.0, -1.16, 0.0]], 'F/C=C/F'),
    'conjugated triene': ([F_, C_, C_, C_, C_, C_, C_, CL_], {(0, 1): 1, (1, 2): 2, (2, 3): 1, (3, 4): 2, (4, 5): 1, (5, 6): 2, (6, 7): 1},
                          [[-2.698, -1.953, -1.476], [-1.448, -1.334, -2.027], [-0.653, -0.635, -1.11], [0.727, -0.197, -1.377],
                           [1.442, 0.527, -0.325], [0.746, 0.78, 0.947], [1.312, 1.459, 2.033], [0.573, 1.353, 3.334]], 'F/C=C/C=C\\C=C\\Cl'),
    'cross-conjugated centre atom': ([F_, C_, C_, C_, C_, CL_, C_, C_, BR_],
                                     {(0, 1): 1, (1, 2): 2, (2, 3): 1, (3, 4): 2, (4, 5): 1, (3, 6): 1, (6, 7): 2, (7, 8): 1},
                                     [[0.725, 0.793, 2.022], [1.851, 0.436, 1.07], [1.524, -0.706, 0.285], [0.133, -0.859, -0.241],
                                      [-0.246, -2.139, -0.838], [-1.712, -2.216, -1.147], [-0.634, 0.357, -0.62], [-0.287, 1.644, -0.209],
                                      [-1.356, 2.691, -0.321]], 'F/C=C\\C(=C\\Cl)\\C=C\\Br'),
    'exocyclic double bond on a ring': ([C_, O_, C_, C_, C_, C_, F_], {(0, 1): 1, (1, 2): 1, (2, 3): 1, (3, 4): 1, (0, 4): 1, (0, 5): 2, (5, 6): 1},
                                        [[-0.123, 0.482, -0.369], [0.24, 0.271, 1.119], [1.334, -0.777, 1.101], [1.624, -1.194, -0.308],
                                         [0.74, -0.428, -1.271], [-1.429, 0.572, -0.659], [-2.387, 1.074, 0.387]], 'C/1(\\OCCC1)=C\\F'),
    'ring double bond': ([C_, C_, C_, C_, C_, C_, F_, CL_], {(0, 1): 2, (1, 2): 1, (2, 3): 1, (3, 4): 1, (4, 5): 1, (0, 5): 1, (0, 6): 1, (1, 7): 1},
                         [[-0.811, 0.22, 0.178], [0.407, 0.532, 0.682], [1.594, -0.201, 0.07], [1.159, -0.683, -1.289], [0.061, -1.675, -1.145],
                          [-1.052, -1.176, -0.311], [-1.993, 1.076, 0.567], [0.635, 1.906, 1.249]], 'C1(=C(CCCC1)Cl)F'),
    'allene': ([F_, C_, C_, C_, CL_], {(0, 1): 1, (1, 2): 2, (2, 3): 2, (3, 4): 1},
               [[0.739, 2.097, 0.1], [-0.33, 1.207, 0.662], [-0.268, -0.119, 0.463], [-0.114, -1.405, 0.113], [-0.028, -1.779, -1.337]], 'FC=C=CCl'),
    'oxime': ([C_, C_, N_, O_], {(0, 1): 1, (1, 2): 2, (2, 3): 1},
              [[0.137, 1.842, -0.542], [-0.071, 0.605, 0.281], [0.008, -0.604, -0.291], [-0.074, -1.842, 0.552]], 'C/C=N/O'),
    'quaternary N+': ([N_, C_, C_, C_, C_, O_, C_, F_], {(0, 1): 1, (0, 2): 1, (2, 3): 1, (0, 4): 1, (4, 5): 1, (0, 6): 1, (6, 7): 1},
                      [[-0.341, 0.167, -0.22], [-0.991, 1.374, -0.828], [1.028, 0.531, 0.273], [1.639, -0.649, 0.969], [-0.23, -0.915, -1.253],
                       [1.088, -0.799, -1.96], [-1.172, -0.323, 0.929], [-1.02, 0.614, 2.091]], '[N@+](C)(CC)(CO)CF'),
    'meso-tartaric skeleton': (*_TARTARIC, [[0.54, 1.499, -0.162], [-0.684, 1.728, 0.339], [1.474, 2.651, -0.398], [0.875, 0.144, -0.716],
                                            [0.024, -0.126, -1.922], [0.615, -0.901, 0.326], [0.957, -2.254, -0.225], [-0.838, -0.874, 0.709],
                                            [-1.708, -1.666, 0.063], [-1.256, -0.201, 1.986]], 'C(=O)(O)[C@H](O)[C@H](O)C(=O)O'),
    'chiral tartaric skeleton': (*_TARTARIC, [[-0.56, -1.132, -0.558], [-0.456, -2.097, 0.366], [-1.887, -0.848, -1.197], [0.661, -0.38, -0.998],
                                              [0.337, 0.435, -2.214], [1.124, 0.522, 0.104], [1.947, -0.26, 1.084], [-0.067, 1.107, 0.81],
                                              [-0.146, 2.44, 0.972], [-0.954, 0.213, 1.631]], 'C(=O)(O)[C@@H](O)[C@H](O)C(=O)O'),
    'centre that is a ring-closure atom': ([C_, O_, C_, C_, C_, F_], {(0, 1): 1, (1, 2): 1, (2, 3): 1, (3, 4): 1, (0, 4): 1, (0, 5): 1},
                                           [[0.163, 0.378, -0.866], [-0.328, 1.151, 0.335], [-0.798, 0.157, 1.369], [-0.623, -1.23, 0.797],
                                            [-0.045, -1.092, -0.591], [1.631, 0.636, -1.043]], '[C@H]1(OCCC1)F'),
}


def example_graphs():
    """[(classes, bonds, pos)] of EXAMPLES, in its order."""
    return [(c, b, np.array(p, dtype=np.float32)) for c, b, p, _ in EXAMPLES.values()]


def assembled(classes, bonds, pos, limits=None):
    """The dict `assemble(keys=True, stereo=)` would return for one graph without dropped atoms, by the restatements alone."""
    assert all(c <= 10 for c in classes)
    r = stereo_of(classes, bonds, pos, limits)
    m = KEY.with_key(KEY.mol_from(classes, bonds))
    _, _, rows = graph_of_rows(*MS.rows_of(classes, bonds))
    at = [rows[(int(a), int(b))] for a, b in m['bond_index'].T.tolist()]
    m['atom_pos'] = torch.as_tensor(np.asarray(pos, dtype=np.float32)).reshape(-1, 3)
    m['stereo'] = dict({'status': r['status'], 'stereo_ok': r['ok'], 'stereo_key': r['stereo_key']}, **dict(zip(M.STEREO_COUNTS, r['counts'].tolist())),
                       atom_parity=r['atom_parity'], atom_label=r['atom_label'], bond_stereo=r['bond_stereo'][at], bond_label=r['bond_label'][at])
    return m


# ---- tools/stereo_host_check.cpp: the cores compiled for the host ---------------------------------------------------------------------------
def run_host_check(exe, cases, work_dir, limits=None, stereo_in=None):
    """cases: [`all_rows` records].  The program perceives every case and writes its isomeric text from what it perceived -- or, for
    the cases of stereo_in {case: (atom_parity, bond_stereo)}, from those values.  Returns one (stereo, text) pair of dicts per case in
    `stereo_of_rows`' and `smiles_of_rows`' forms."""
    limits = M.StereoLimits() if limits is None else limits
    stereo_in = stereo_in or {}
    path = os.path.join(str(work_dir), 'stereo_cases.txt')
    listed = []
    with open(path, 'w') as fh:
        fh.write(' '.join(str(v) for v in MS.padded_valences(M.SMILES_VALENCES)) + '\n')
        fh.write('%s %s %d\n' % (float(limits.vol_min).hex(), float(limits.planar_min).hex(), limits.max_undefined))
        for c, m in enumerate(cases):
            n = len(m.cls)
            rows, a, b = MS.listed_pairs(n, m.order)
            listed.append(rows)
            given = stereo_in.get(c)
            fh.write('%d %d %d %d %d %d\n' % (n, 12 * max(n, 8), m.kekule_status, rows.size, int(m.key) & M64, given is not None))
            for i in range(n):
                fh.write('%d %d %d %d %s %s %s %d\n' % (m.cls[i], m.hcount[i], m.charge[i], int(m.colour[i]) & M64, *(MS.hex32(x) for x in m.pos[i]),
                                                         given[0][i] if given is not None else 0))
            for x, y, r in zip(a, b, rows):
                fh.write('%d %d %d %d %d %d\n' % (x, y, m.order[r], m.kekule_order[r], m.ring_size[r], given[1][r] if given is not None else 0))
    out = MS.run_program(exe, path)
    got = []
    for c, (case, rows) in enumerate(zip(cases, listed)):
        n, hh = len(case.cls), len(case.order)
        head, atoms, pairs, shead, text, ranks = (out[6 * c + k] for k in range(6))
        head, atoms, pairs, shead = ([int(v) for v in x.split()] for x in (head, atoms, pairs, shead))
        st = {'status': head[0], 'stereo_key': head[1], 'counts': np.array(head[2:], dtype=np.int32),
              'atom_parity': np.array(atoms[0::2], dtype=np.int8).reshape(n), 'atom_label': np.array(atoms[1::2], dtype=np.int8).reshape(n),
              'bond_stereo': np.zeros(hh, dtype=np.int8), 'bond_label': np.zeros(hh, dtype=np.int8)}
        st['bond_stereo'][rows], st['bond_label'][rows] = pairs[0::2], pairs[1::2]
        tx = {'text': text, 'status': shead[0], 'ok': shead[0] & M.SMILES_FAIL_MASK == 0, 'length': shead[1],
              'counts': np.array(shead[2:10], dtype=np.int32), 'stereo_counts': np.array(shead[10:], dtype=np.int32),
              'atom_rank': np.array([int(v) for v in ranks.split()], dtype=np.int16)}
        assert len(text) == shead[1]
        got.append((st, tx))
    return got
