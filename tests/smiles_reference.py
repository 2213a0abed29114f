"""Plain restatement of the SMILES writer (DESIGN.md 2.9 "SMILES"; phoregen_amd/molecule.py, csrc/mol_smiles.hip) for the tests, and an
independent reader of what it emits.

The writer is written from the definition's text in another form than the kernel: recursive, over dicts and sets, strings joined as
the definition's `visit(v)` joins them -- no stack, no bit masks, no prefix sum.  The reader parses the emitted subset of OpenSMILES
(bare and bracket atoms, '=', '#', branches, ring-closure labels with '%nn', '.', implicit hydrogens by the notation's own valence
rule) and knows nothing of the writer.  Neither holds device code; they share nothing with the kernel but the named constants and
tables of phoregen_amd.molecule.  Also here: the hand-checked examples, and the case format of tools/smiles_host_check.cpp."""
import os
import sys

import numpy as np

import kekule_reference as K
import mol_support as MS
from mol_support import C_, N_, O_, SI_, I_
from phoregen_amd import molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

BOND_SYMBOL = {1: '', 2: '=', 3: '#'}


class RingLabels(Exception):
    """More than SMILES_MAX_LABEL labels would be in use at once."""


def implicit_h(z, bond_sum):
    """The notation's rule for a bare atom of atomic number z."""
    fits = [t for t in M.SMILES_VALENCES[z] if t >= bond_sum]
    return min(fits) - bond_sum if fits else 0


def atom_token(z, bond_sum, h, q):
    """(text, is a bracket atom)"""
    if M.SMILES_VALENCES[z] and q == 0 and implicit_h(z, bond_sum) == h:
        return M.ELEMENT_SYMBOL[z], False
    return '[' + M.ELEMENT_SYMBOL[z] + ('H' if h >= 1 else '') + (str(h) if h >= 2 else '') + ('+' if q == 1 else '') + ']', True


def label_text(label):
    return str(label) if label <= 9 else '%%%02d' % label


def write_graph(elements, bonds, hcount, charge):
    """The definition, for one graph given as dicts over the kept atoms' local indices: elements {i: z}, bonds {(a, b): 1 | 2 | 3} with
    a < b, hcount {i: h}, charge {i: q}.  Returns {'text', 'rank' {i: position}, 'components', 'ring_closures', 'branches',
    'max_label', 'bracket_atoms'}; raises RingLabels."""
    nbr = {i: {} for i in elements}
    for (a, b), o in bonds.items():
        nbr[a][b] = nbr[b][a] = o
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    rank, parent, children = {}, {}, {i: [] for i in elements}

    def walk(v):                                                       # the traversal: who is whose child, in which order
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
    # a bond that is not a tree bond joins an atom to one of its ancestors: it opens at the ancestor and closes at the descendant
    opens, closes = {i: [] for i in elements}, {i: [] for i in elements}
    for (a, b) in bonds:
        if parent[a] != b and parent[b] != a:
            anc, desc = (a, b) if rank[a] < rank[b] else (b, a)
            opens[anc].append(desc)
            closes[desc].append(anc)
    in_use, label, stats = set(), {}, {'max_label': 0, 'bracket_atoms': 0, 'branches': 0}

    def visit(v):
        token, bracket = atom_token(elements[v], sum(nbr[v].values()), hcount[v], charge[v])
        stats['bracket_atoms'] += bracket
        text = (BOND_SYMBOL[nbr[v][parent[v]]] if parent[v] is not None else '') + token
        for a in sorted(closes[v]):
            text += label_text(label[(a, v)])
        for d in sorted(opens[v]):
            free = [k for k in range(1, M.SMILES_MAX_LABEL + 1) if k not in in_use]
            if not free:
                raise RingLabels()
            label[(v, d)] = free[0]
            in_use.add(free[0])
            stats['max_label'] = max(stats['max_label'], free[0])
            text += BOND_SYMBOL[nbr[v][d]] + label_text(free[0])
        for a in closes[v]:                                            # in use until after the whole group of the atom where it closes
            in_use.discard(label[(a, v)])
        for c in children[v][:-1]:
            stats['branches'] += 1
            text += '(' + visit(c) + ')'
        if children[v]:
            text += visit(children[v][-1])
        return text

    text = '.'.join(visit(r) for r in roots)
    return dict(stats, text=text, rank=rank, components=len(roots), ring_closures=sum(len(v) for v in opens.values()))


def smiles_of_rows(cls, kekule_order, hcount, charge, kekule_status=0, capacity=None):
    """The restatement's answer for one graph as the device holds it: cls [n] (-1 = dropped), kekule_order [n (n - 1) / 2], hcount,
    charge [n], the graph's Kekulé status; capacity None = 8 * max(n, 8).  Returns 'text' (str), 'status', 'ok', 'length', 'counts'
    (int32 [8]) and 'atom_rank' (int16 [n])."""
    cls, kek = [int(c) for c in cls], [int(o) for o in kekule_order]
    n = len(cls)
    capacity = 8 * max(n, 8) if capacity is None else capacity
    failed = lambda bit: {'text': '', 'status': bit, 'ok': False, 'length': 0, 'counts': np.zeros(8, dtype=np.int32),   # noqa: E731
                          'atom_rank': np.full(n, -1, dtype=np.int16)}
    if kekule_status & M.KEKULE_FAILED:
        return failed(M.SMILES_NO_KEKULE)
    elements = {i: ATOM_TYPES[c] for i, c in enumerate(cls) if 0 <= c <= 10}
    bonds = {p: kek[row] for p, row in MS.pair_walk(cls, kek, (1, 2, 3)).rows.items()}
    try:
        w = write_graph(elements, bonds, {i: int(hcount[i]) for i in elements}, {i: int(charge[i]) for i in elements})
    except RingLabels:
        return failed(M.SMILES_RING_LABELS)
    text = w['text']
    fits = len(text) <= capacity
    status = (0 if fits else M.SMILES_TOO_LONG) | (M.SMILES_DISCONNECTED if '.' in text else 0) | (0 if elements else M.SMILES_EMPTY)
    status |= M.SMILES_BRACKET if w['bracket_atoms'] else 0
    counts = {'length': len(text), 'atoms': len(elements), 'bonds': len(bonds), 'components': w['components'],
              'ring_closures': w['ring_closures'], 'branches': w['branches'], 'max_label': w['max_label'], 'bracket_atoms': w['bracket_atoms']}
    assert w['branches'] == text.count('(') == text.count(')') and text.count('[') == w['bracket_atoms']
    return {'text': text if fits else '', 'status': status, 'ok': fits, 'length': len(text) if fits else 0,
            'counts': np.array([counts[k] for k in M.SMILES_COUNTS], dtype=np.int32),
            'atom_rank': np.array([w['rank'][i] if fits and i in elements else -1 for i in range(n)], dtype=np.int16)}


# ---- the reader -------------------------------------------------------------------------------------------------------------------------
_BARE = sorted((sym for z, sym in M.ELEMENT_SYMBOL.items() if M.SMILES_VALENCES[z]), key=len, reverse=True)   # two letters first
_Z = {sym: z for z, sym in M.ELEMENT_SYMBOL.items()}
_ORDER = {'=': 2, '#': 3}


def read_smiles(text):
    """Parse the emitted subset of OpenSMILES.  Returns (atoms, bonds): atoms = [(z, hydrogens, charge)] in text order, bonds =
    {(i, j): order} with i < j.  Anything outside the subset, an unclosed ring or branch, a bond symbol with nothing to bond, a label
    closed on its own atom or a second bond between two atoms raises ValueError."""
    atoms, explicit, bonds = [], [], {}
    stack, prev, pending, open_rings = [], None, None, {}
    k = 0

    def bond(i, j, order):
        key = (min(i, j), max(i, j))
        if i == j or key in bonds:
            raise ValueError('%r: second bond or self bond %r' % (text, key))
        bonds[key] = order

    def add_atom(z, h, q):
        nonlocal prev, pending
        atoms.append((z, h, q))
        if prev is not None:
            bond(prev, len(atoms) - 1, pending or 1)
        elif pending is not None:
            raise ValueError('%r: bond symbol without an atom before it' % text)
        prev, pending = len(atoms) - 1, None

    while k < len(text):
        ch = text[k]
        if ch == '[':
            end = text.index(']', k)
            body = text[k + 1:end]
            sym = next((s for s in sorted(_Z, key=len, reverse=True) if body.startswith(s)), None)
            if sym is None:
                raise ValueError('%r: bracket atom %r' % (text, body))
            rest, h, q = body[len(sym):], 0, 0
            if rest.startswith('H'):
                digits = ''
                rest = rest[1:]
                while rest and rest[0].isdigit():
                    digits, rest = digits + rest[0], rest[1:]
                h = int(digits) if digits else 1
            if rest == '+':
                q, rest = 1, ''
            if rest:
                raise ValueError('%r: bracket atom %r' % (text, body))
            add_atom(_Z[sym], h, q)
            explicit.append(True)
            k = end + 1
        elif ch in _ORDER:
            if pending is not None or prev is None:
                raise ValueError('%r: bond symbol at %d' % (text, k))
            pending = _ORDER[ch]
            k += 1
        elif ch == '(':
            if prev is None or pending is not None:
                raise ValueError('%r: branch at %d' % (text, k))
            stack.append(prev)
            k += 1
        elif ch == ')':
            if not stack or pending is not None:
                raise ValueError('%r: ) at %d' % (text, k))
            prev = stack.pop()
            k += 1
        elif ch == '.':
            if stack or pending is not None or prev is None:
                raise ValueError('%r: . at %d' % (text, k))
            prev = None
            k += 1
        elif ch.isdigit() or ch == '%':
            if ch == '%':
                if not text[k + 1:k + 3].isdigit() or len(text[k + 1:k + 3]) != 2:
                    raise ValueError('%r: label at %d' % (text, k))
                lab, k = int(text[k + 1:k + 3]), k + 3
            else:
                lab, k = int(ch), k + 1
            if prev is None:
                raise ValueError('%r: label without an atom' % text)
            if lab in open_rings:
                other, order = open_rings.pop(lab)
                if order is not None and pending is not None and order != pending:
                    raise ValueError('%r: label %d with two bond orders' % (text, lab))
                bond(other, prev, pending or order or 1)
            else:
                open_rings[lab] = (prev, pending)
            pending = None
        else:
            sym = next((s for s in _BARE if text.startswith(s, k)), None)
            if sym is None:
                raise ValueError('%r: %r at %d' % (text, ch, k))
            add_atom(_Z[sym], None, 0)
            explicit.append(False)
            k += len(sym)
    if stack or open_rings or pending is not None:
        raise ValueError('%r: unclosed branch, ring or bond' % text)
    total = [0] * len(atoms)
    for (i, j), o in bonds.items():
        total[i] += o
        total[j] += o
    atoms = [(z, h if ex else implicit_h(z, total[i]), q) for i, ((z, h, q), ex) in enumerate(zip(atoms, explicit))]
    return atoms, bonds


def molecule_in_text_order(cls, kekule_order, hcount, charge, atom_rank):
    """The molecule the text must read back to: (atoms, bonds) as `read_smiles` returns them, under atom k <-> the atom of rank k."""
    cls, rank = [int(c) for c in cls], [int(r) for r in atom_rank]
    n = len(cls)
    kept = [i for i in range(n) if 0 <= cls[i] <= 10]
    assert sorted(rank[i] for i in kept) == list(range(len(kept))) and all(rank[i] == -1 for i in range(n) if i not in kept), rank
    by_rank = sorted(kept, key=lambda i: rank[i])
    atoms = [(ATOM_TYPES[cls[i]], int(hcount[i]), int(charge[i])) for i in by_rank]
    w = MS.pair_walk(cls, kekule_order, (1, 2, 3))
    return atoms, {(min(rank[a], rank[b]), max(rank[a], rank[b])): w.order[row] for (a, b), row in w.rows.items()}


def check_read_back(text, cls, kekule_order, hcount, charge, atom_rank, where=''):
    """read_back(text) == the molecule, exactly: elements, hydrogens, charges and the bond set with its orders."""
    got, want = read_smiles(text), molecule_in_text_order(cls, kekule_order, hcount, charge, atom_rank)
    assert got[0] == want[0], (where, text, 'atoms', got[0], want[0])
    assert got[1] == want[1], (where, text, 'bonds', sorted(set(got[1].items()) ^ set(want[1].items()))[:8])
    return got


def formula_of_text(text):
    """`formula_of` on the atoms read back."""
    atoms, _ = read_smiles(text)
    return M.formula_of([z for z, _, _ in atoms], [h for _, h, _ in atoms], sum(q for _, _, q in atoms))[0]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def kekule_rows(classes, bonds, allow_charged=True):
    """(cls, kekule_order, hcount, charge, kekule_status) of one (classes, {(a, b): bond class}) graph by the Kekulé restatement."""
    cls, order = MS.rows_of(classes, bonds)
    r = K.kekule_of_rows(cls, order, allow_charged)
    return cls, r['kekule_order'], r['hcount'], r['charge'], int(r['status'])


def ring(n, off=0):
    return K.cycle(n, 1, off)


# name: (classes, bonds with orders 1..3 (or aromatic 4, resolved by the Kekulé form), text) -- the texts were checked by hand
EXAMPLES = {
    'ethanol': ([C_, C_, O_], {(0, 1): 1, (1, 2): 1}, 'CCO'),
    'isobutene': ([C_] * 4, {(0, 1): 2, (1, 2): 1, (1, 3): 1}, 'C=C(C)C'),
    'cyclohexene': ([C_] * 6, {**ring(6), (0, 5): 2}, 'C=1CCCCC1'),
    'pyrrole': ([N_] + [C_] * 4, K.cycle(5), 'N1C=CC=C1'),
    'silanol': ([SI_, O_], {(0, 1): 1}, '[SiH3]O'),
    'tetramethylammonium': ([N_] + [C_] * 4, {(0, i): 1 for i in range(1, 5)}, '[N+](C)(C)(C)C'),
    'two lone atoms': ([C_, O_], {}, 'C.O'),
    'two cyclopropanes joined by a bond': ([C_] * 6, {(0, 1): 1, (1, 2): 1, (0, 2): 1, (2, 3): 1, (3, 4): 1, (4, 5): 1, (3, 5): 1}, 'C1CC1C1CC1'),
    'spiro[2.2]pentane': ([C_] * 5, {(0, 1): 1, (1, 2): 1, (0, 2): 1, (2, 3): 1, (3, 4): 1, (2, 4): 1}, 'C1CC12CC2'),
    'norbornane': ([C_] * 7, {**ring(6), (0, 6): 1, (3, 6): 1}, 'C12CCC(CC1)C2'),
    'tetrahedrane skeleton': ([C_] * 4, {(a, b): 1 for a in range(4) for b in range(a + 1, 4)}, 'C12C3C1C23'),
    'dimethyl ether with a dropped atom': ([C_, 11, O_, C_], {(0, 2): 1, (2, 3): 1}, 'COC'),
    'iodine between two carbons': ([C_, I_, C_], {(0, 1): 1, (1, 2): 1}, 'C[IH]C'),
    'acetonitrile': ([C_, C_, N_], {(0, 1): 1, (1, 2): 3}, 'CC#N'),
}


def label_boundary(extra):
    """A chain 0..127 of carbons with atom 0 also bonded to atoms 2 .. 2 + extra - 1: `extra` ring closures open at once."""
    return [C_] * 128, {**K.chain(128, 1), **{(0, i): 1 for i in range(2, 2 + extra)}}


# ---- tools/smiles_host_check.cpp: the kernel's core compiled for the host ----------------------------------------------------------------
def run_host_check(exe, cases, work_dir):
    """cases: [(cls, kekule_order, hcount, charge, kekule_status, capacity or None)] -> one dict per case in `smiles_of_rows`' form."""
    path = os.path.join(str(work_dir), 'smiles_cases.txt')
    with open(path, 'w') as fh:
        fh.write(' '.join(str(v) for v in MS.padded_valences(M.SMILES_VALENCES)) + '\n')
        for cls, kek, h, q, kstatus, capacity in cases:
            n = len(cls)
            rows, a, b = MS.listed_pairs(n, kek)
            fh.write('%d %d %d %d\n' % (n, 8 * max(n, 8) if capacity is None else capacity, kstatus, rows.size))
            for arr in (cls, h, q):
                fh.write(' '.join(str(int(x)) for x in arr) + '\n')
            fh.write(' '.join('%d %d %d' % (x, y, kek[r]) for x, y, r in zip(a, b, rows)) + '\n')
    out = MS.run_program(exe, path)
    got = []
    for c in range(len(cases)):
        head, text, ranks = [int(v) for v in out[3 * c].split()], out[3 * c + 1], [int(v) for v in out[3 * c + 2].split()]
        got.append({'text': text, 'status': head[0], 'ok': head[0] & M.SMILES_FAIL_MASK == 0, 'length': head[1],
                    'counts': np.array(head[2:], dtype=np.int32), 'atom_rank': np.array(ranks, dtype=np.int16)})
        assert len(text) == head[1]
    return got


def same_answer(got, want, where=''):
    """Byte for byte: text, status, length, counts and ranks."""
    assert got['text'] == want['text'], (where, got['text'], want['text'])
    assert int(got['status']) == want['status'] and int(got['length']) == want['length'], (where, got['status'], want['status'])
    assert np.asarray(got['counts']).tolist() == want['counts'].tolist(), (where, dict(zip(M.SMILES_COUNTS, zip(np.asarray(got['counts']).tolist(), want['counts'].tolist()))))
    assert np.asarray(got['atom_rank']).tolist() == want['atom_rank'].tolist(), (where, 'ranks')
