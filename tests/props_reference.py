"""Plain restatement of the property descriptors (DESIGN.md 2.9 "Properties"; phoregen_amd/properties.py, csrc/mol_props.hip,
csrc/props_core.h) for the tests, written from the text in another form than the kernel: neighbour dicts, one dict of field values per
atom that is packed at the end, Python integers.  No device code; it shares nothing with the kernel but the tables and limits it is
handed.  The Kekulé form and the rings are inputs: on the CPU they come from kekule_reference / ring_reference, on the GPU from the
kernels that the property kernel reads.  Also here: the named molecules with their hand-written answers, the random family, and the
case format of tools/props_host_check.cpp."""
import os

import numpy as np

import kekule_reference as K
import mol_support as MS
import ring_reference as G
from mol_support import B_, C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, I_, chain, cycle  # noqa: F401

# the word, from the table of the text: (field, first bit, bits)
FIELDS = (('el', 0, 4), ('h', 4, 3), ('q', 7, 1), ('deg', 8, 3), ('arom', 11, 1), ('n_dbl', 12, 2), ('triple', 14, 1), ('ring', 15, 1),
          ('ring3', 16, 1), ('nb_het', 17, 3), ('nb_arom', 20, 2), ('dbl_o', 22, 1), ('dbl_het', 23, 1), ('nb_dbl_het', 24, 1),
          ('nb_hal', 25, 2), ('nb_no', 27, 3))
COUNTS = ('heavy_atoms', 'hydrogens', 'carbons', 'sp3_carbons', 'heteroatoms', 'halogens', 'nhoh', 'no_count', 'rotatable', 'amide_bonds',
          'aromatic_atoms', 'ring_atoms', 'net_charge', 'untyped', 'violations', 'reserved')
HALOGENS, NOPS = (F_, CL_, BR_, I_), (N_, O_, P_, S_)
NO_KEKULE, LIMITS, UNTYPED = 1, 2, 4
KEKULE_FAILED = 1
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
NO_LIMITS = [(INT_MIN, INT_MAX)] * 9
# atomic weights times 1000, the eleven classes and hydrogen (the values of phoregen_amd.molecule.ATOMIC_WEIGHT, written out)
WEIGHTS = [10810, 12011, 14007, 15999, 18998, 28085, 30974, 32060, 35450, 79904, 126904, 1008]


def pack(fields):
    """A word from {field: value}; a value above its field's width saturates."""
    word = 0
    for name, first, bits in FIELDS:
        word |= min(int(fields.get(name, 0)), (1 << bits) - 1) << first
    assert not set(fields) - {f[0] for f in FIELDS}
    return word


def unpack(word):
    return {name: (word >> first) & ((1 << bits) - 1) for name, first, bits in FIELDS}


def atom_fields(cls, order, kek_order, hcount, charge, ring_size, atom_ring):
    """Per atom the unsaturated field values (None for a dropped atom), and the bonds {(a, b): (single, double, triple, ring bond)}."""
    kept, nbrs, rows, order = MS.pair_walk(cls, order)
    n = len(kept)
    cls = [int(c) for c in cls]
    bond = {}
    for (a, b), row in rows.items():
        k, four = int(kek_order[row]), order[row] == 4
        bond[(a, b)] = bond[(b, a)] = {'single': k == 1 and not four, 'double': k == 2 and not four, 'triple': k == 3,
                                       'arom': four and int(ring_size[row]) > 0, 'ring': int(ring_size[row]) > 0}
    first = []
    for i in range(n):
        if not kept[i]:
            first.append(None)
            continue
        mine = [(z, bond[(i, z)]) for z in nbrs[i]]
        doubles = [z for z, bd in mine if bd['double']]
        first.append({'el': cls[i], 'h': int(hcount[i]), 'q': int(int(charge[i]) > 0), 'deg': len(mine),
                      'arom': int(any(bd['arom'] for _, bd in mine)), 'n_dbl': len(doubles), 'triple': int(any(bd['triple'] for _, bd in mine)),
                      'ring': int(int(atom_ring[i]) > 0), 'ring3': int(int(atom_ring[i]) == 3), 'nb_het': sum(cls[z] != C_ for z, _ in mine),
                      'dbl_o': int(any(cls[z] == O_ for z in doubles)), 'dbl_het': int(any(cls[z] in NOPS for z in doubles)),
                      'nb_hal': sum(cls[z] in HALOGENS for z, _ in mine), 'nb_no': sum(cls[z] in (N_, O_) for z, _ in mine)})
    for i in range(n):
        if first[i] is not None:
            first[i]['nb_arom'] = sum(first[z]['arom'] for z in nbrs[i])
            first[i]['nb_dbl_het'] = int(any(bond[(i, z)]['single'] and first[z]['dbl_het'] for z in nbrs[i]))
    return first, {k: v for k, v in bond.items() if k[0] < k[1]}


def first_row(rows, word):
    return next((r for r, (mask, value, _, _) in enumerate(rows) if word & mask == value), None)


def properties_of_rows(cls, order, kek_order, hcount, charge, kek_status, ring_size, atom_ring, tables=(), pairs=NO_LIMITS,
                       max_violations=0, weights=WEIGHTS):
    """Every output of one graph.  tables: [rows] with rows = [(mask, value, atom, per_h)]; pairs: nine (lo, hi)."""
    n = len(cls)
    out = {'atom_env': np.full(n, -1, dtype=np.int32), 'atom_row': np.full((4, n), 255, dtype=np.uint8), 'sums': np.zeros(4, dtype=np.int32),
           'counts': np.zeros(16, dtype=np.int32), 'weight_milli': 0, 'violated': 0, 'status': NO_KEKULE, 'ok': False}
    if int(kek_status) & KEKULE_FAILED:
        return out
    fields, bonds = atom_fields(cls, order, kek_order, hcount, charge, ring_size, atom_ring)
    c, sums, weight = dict.fromkeys(COUNTS, 0), [0, 0, 0, 0], 0
    words = {}
    for i, f in enumerate(fields):
        if f is None:
            continue
        words[i] = word = pack(f)
        out['atom_env'][i] = word
        g, h = unpack(word), int(hcount[i])                            # (the counts read the word; the hydrogens are the atom's own)
        c['heavy_atoms'] += 1
        c['hydrogens'] += h
        c['carbons'] += g['el'] == C_
        c['sp3_carbons'] += g['el'] == C_ and not g['arom'] and g['n_dbl'] == 0 and not g['triple']
        c['heteroatoms'] += g['el'] != C_
        c['halogens'] += g['el'] in HALOGENS
        c['nhoh'] += h if g['el'] in (N_, O_) else 0
        c['no_count'] += g['el'] in (N_, O_)
        c['aromatic_atoms'] += g['arom']
        c['ring_atoms'] += g['ring']
        c['net_charge'] += int(charge[i])
        weight += weights[g['el']] + h * weights[11]
        for t, rows in enumerate(tables):
            r = first_row(rows, word)
            if r is None:
                c['untyped'] += 1
            else:
                out['atom_row'][t, i] = r
                sums[t] += rows[r][2] + h * rows[r][3]
    for (a, b), bd in bonds.items():
        if not bd['single'] or bd['ring']:
            continue
        fa, fb = unpack(words[a]), unpack(words[b])
        if any(x['el'] == C_ and x['dbl_o'] and y['el'] == N_ for x, y in ((fa, fb), (fb, fa))):
            c['amide_bonds'] += 1
        elif fa['deg'] >= 2 and fb['deg'] >= 2 and not fa['triple'] and not fb['triple']:
            c['rotatable'] += 1
    quantities = [weight, c['heavy_atoms'], c['nhoh'], c['no_count'], c['rotatable']] + sums
    assert all(INT_MIN <= q <= INT_MAX for q in quantities)
    violated = sum(1 << k for k, (q, (lo, hi)) in enumerate(zip(quantities, pairs)) if q < lo or q > hi)
    c['violations'] = bin(violated).count('1')
    status = (LIMITS if c['violations'] > max_violations else 0) | (UNTYPED if c['untyped'] else 0)
    out.update(sums=np.array(sums, dtype=np.int32), counts=np.array([c[k] for k in COUNTS], dtype=np.int32), weight_milli=weight,
               violated=violated, status=status, ok=not status & (NO_KEKULE | LIMITS))
    return out


def cpu_inputs(classes, bonds):
    """(cls, order, kek_order, hcount, charge, kekule status, ring_size, atom_ring) of one graph from the restatements of the Kekulé
    form and the rings."""
    cls, order = K.rows_of(classes, dict(bonds))
    kk, rr = K.kekule_of_rows(cls, order), G.rings_of_rows(cls, order)
    return cls, order, kk['kekule_order'], kk['hcount'], kk['charge'], int(kk['status']), rr['ring_size'], rr['atom_ring']


def properties_of(classes, bonds, tables=(), pairs=NO_LIMITS, max_violations=0):
    return properties_of_rows(*cpu_inputs(classes, bonds), tables, pairs, max_violations)


# ---- the named molecules: classes, bonds, and by hand: the fields of every atom's word that are not 0, the row every atom takes in
# HAND_ROWS (None: no row), the counts that are not 0, and the weight times 1000 -----------------------------------------------------------
# HAND_ROWS as (fields, atom, per_h) in units of 1e-4: aromatic C; C with a double bond to O; any C; N next to C=O; O with one H; aromatic N
HAND_ROWS = [({'el': C_, 'arom': 1}, 10000, 1000), ({'el': C_, 'dbl_o': 1}, 20000, 0), ({'el': C_}, 5000, 2500),
             ({'el': N_, 'nb_dbl_het': 1}, -10000, 5000), ({'el': O_, 'h': 1}, -5000, 1250), ({'el': N_, 'arom': 1}, 30000, 0)]


def rows_from_fields(spec):
    """[(mask, value, atom, per_h)] from [({field: value}, atom, per_h)]: the mask covers the named fields."""
    width = {name: (first, bits) for name, first, bits in FIELDS}
    return [(sum(((1 << width[k][1]) - 1) << width[k][0] for k in f), pack(f), a, p) for f, a, p in spec]


def _f(el, **fields):
    return dict(el=el, **fields)


_CH3, _CH2 = _f(C_, h=3, deg=1), _f(C_, h=2, deg=2)
_CH3_CO = _f(C_, h=3, deg=1, nb_dbl_het=1)                             # (the methyl next to C=O: any single-bonded neighbour of it has the bit)
_CH3X = _f(C_, h=3, deg=1, nb_het=1, nb_no=1)
_CARBONYL_C = _f(C_, deg=3, n_dbl=1, nb_het=2, dbl_o=1, dbl_het=1, nb_no=2)
_CARBONYL_O = _f(O_, deg=1, n_dbl=1)
_CH_AR = _f(C_, h=1, deg=2, arom=1, ring=1, nb_arom=2)
_CH_AR_N = _f(C_, h=1, deg=2, arom=1, ring=1, nb_arom=2, nb_het=1, nb_no=1)
_RING6 = cycle(6, 4)
NAMED = {
    'ethanol': ([C_, C_, O_], chain(3, 1), [_CH3, _f(C_, h=2, deg=2, nb_het=1, nb_no=1), _f(O_, h=1, deg=1)], [2, 2, 4],
                dict(heavy_atoms=3, hydrogens=6, carbons=2, sp3_carbons=2, heteroatoms=1, nhoh=1, no_count=1), 46069),
    'acetic acid': ([C_, C_, O_, O_], {(0, 1): 1, (1, 2): 2, (1, 3): 1}, [_CH3_CO, _CARBONYL_C, _CARBONYL_O, _f(O_, h=1, deg=1, nb_dbl_het=1)],
                    [2, 1, None, 4], dict(heavy_atoms=4, hydrogens=4, carbons=2, sp3_carbons=1, heteroatoms=2, nhoh=1, no_count=2), 60052),
    'acetamide': ([C_, C_, O_, N_], {(0, 1): 1, (1, 2): 2, (1, 3): 1}, [_CH3_CO, _CARBONYL_C, _CARBONYL_O, _f(N_, h=2, deg=1, nb_dbl_het=1)],
                  [2, 1, None, 3], dict(heavy_atoms=4, hydrogens=5, carbons=2, sp3_carbons=1, heteroatoms=2, nhoh=2, no_count=2, amide_bonds=1),
                  59068),
    'N-methylacetamide': ([C_, C_, O_, N_, C_], {(0, 1): 1, (1, 2): 2, (1, 3): 1, (3, 4): 1},
                          [_CH3_CO, _CARBONYL_C, _CARBONYL_O, _f(N_, h=1, deg=2, nb_dbl_het=1), _CH3X], [2, 1, None, 3, 2],
                          dict(heavy_atoms=5, hydrogens=7, carbons=3, sp3_carbons=2, heteroatoms=2, nhoh=1, no_count=2, amide_bonds=1), 73095),
    # the ester's C-O is a single bond between two atoms of degree 2 and more, outside a ring: rotatable by this definition
    'methyl acetate': ([C_, C_, O_, O_, C_], {(0, 1): 1, (1, 2): 2, (1, 3): 1, (3, 4): 1},
                       [_CH3_CO, _CARBONYL_C, _CARBONYL_O, _f(O_, deg=2, nb_dbl_het=1), _CH3X], [2, 1, None, None, 2],
                       dict(heavy_atoms=5, hydrogens=6, carbons=3, sp3_carbons=2, heteroatoms=2, no_count=2, rotatable=1), 74079),
    'benzene': ([C_] * 6, _RING6, [_CH_AR] * 6, [0] * 6, dict(heavy_atoms=6, hydrogens=6, carbons=6, aromatic_atoms=6, ring_atoms=6), 78114),
    'pyridine': ([N_] + [C_] * 5, _RING6, [_f(N_, deg=2, arom=1, ring=1, nb_arom=2), _CH_AR_N, _CH_AR, _CH_AR, _CH_AR, _CH_AR_N],
                 [5, 0, 0, 0, 0, 0], dict(heavy_atoms=6, hydrogens=5, carbons=5, heteroatoms=1, no_count=1, aromatic_atoms=6, ring_atoms=6), 79102),
    'pyrrole': ([N_] + [C_] * 4, cycle(5, 4), [_f(N_, h=1, deg=2, arom=1, ring=1, nb_arom=2), _CH_AR_N, _CH_AR, _CH_AR, _CH_AR_N],
                [5, 0, 0, 0, 0], dict(heavy_atoms=5, hydrogens=5, carbons=4, heteroatoms=1, nhoh=1, no_count=1, aromatic_atoms=5, ring_atoms=5),
                67091),
    'phenol': ([C_] * 6 + [O_], {**_RING6, (0, 6): 1},
               [_f(C_, deg=3, arom=1, ring=1, nb_arom=2, nb_het=1, nb_no=1)] + [_CH_AR] * 5 + [_f(O_, h=1, deg=1, nb_arom=1)], [0] * 6 + [4],
               dict(heavy_atoms=7, hydrogens=6, carbons=6, heteroatoms=1, nhoh=1, no_count=1, aromatic_atoms=6, ring_atoms=6), 94113),
    'acetonitrile': ([C_, C_, N_], {(0, 1): 1, (1, 2): 3}, [_CH3, _f(C_, deg=2, triple=1, nb_het=1, nb_no=1), _f(N_, deg=1, triple=1)],
                     [2, 2, None], dict(heavy_atoms=3, hydrogens=3, carbons=2, sp3_carbons=1, heteroatoms=1, no_count=1), 41053),
    'chlorobenzene': ([C_] * 6 + [CL_], {**_RING6, (0, 6): 1},
                      [_f(C_, deg=3, arom=1, ring=1, nb_arom=2, nb_het=1, nb_hal=1)] + [_CH_AR] * 5 + [_f(CL_, deg=1, nb_arom=1)], [0] * 6 + [None],
                      dict(heavy_atoms=7, hydrogens=5, carbons=6, heteroatoms=1, halogens=1, aromatic_atoms=6, ring_atoms=6), 112556),
    'oxirane': ([O_, C_, C_], cycle(3, 1), [_f(O_, deg=2, ring=1, ring3=1)] + [_f(C_, h=2, deg=2, ring=1, ring3=1, nb_het=1, nb_no=1)] * 2,
                [None, 2, 2], dict(heavy_atoms=3, hydrogens=4, carbons=2, sp3_carbons=2, heteroatoms=1, no_count=1, ring_atoms=3), 44053),
    'dimethyl sulfone': ([C_, S_, O_, O_, C_], {(0, 1): 1, (1, 2): 2, (1, 3): 2, (1, 4): 1},
                         [_f(C_, h=3, deg=1, nb_het=1, nb_dbl_het=1), _f(S_, deg=4, n_dbl=2, nb_het=2, dbl_o=1, dbl_het=1, nb_no=2)]
                         + [_f(O_, deg=1, n_dbl=1, nb_het=1, dbl_het=1)] * 2 + [_f(C_, h=3, deg=1, nb_het=1, nb_dbl_het=1)], [2, None, None, None, 2],
                         dict(heavy_atoms=5, hydrogens=6, carbons=2, sp3_carbons=2, heteroatoms=3, no_count=2), 94128),
    # three methyls on N: the Kekulé form fills N's valence 3, so this is what it makes of trimethylammonium's heavy atoms -- no
    # hydrogen on N and no charge; the charged N is the four-valent one of the next entry
    'trimethylammonium': ([N_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1}, [_f(N_, deg=3)] + [_CH3X] * 3, [None, 2, 2, 2],
                          dict(heavy_atoms=4, hydrogens=9, carbons=3, sp3_carbons=3, heteroatoms=1, no_count=1), 59112),
    'tetramethylammonium': ([N_, C_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1}, [_f(N_, q=1, deg=4)] + [_CH3X] * 4,
                            [None, 2, 2, 2, 2], dict(heavy_atoms=5, hydrogens=12, carbons=4, sp3_carbons=4, heteroatoms=1, no_count=1, net_charge=1),
                            74147),
    'butane': ([C_] * 4, chain(4, 1), [_CH3, _CH2, _CH2, _CH3], [2] * 4, dict(heavy_atoms=4, hydrogens=10, carbons=4, sp3_carbons=4, rotatable=1),
               58124),
}


def named_graphs():
    return [(v[0], v[1]) for v in NAMED.values()]


# ---- the random family: valence-clean graphs of up to FAMILY_MAX atoms, grown atom by atom under the elements' valences, and a few
# designed ones that set the high bits of the wide fields ----------------------------------------------------------------------------------
FAMILY_SEED, FAMILY_GRAPHS, FAMILY_MAX = 20261020, 36, 40
VALENCE = {B_: 3, C_: 4, N_: 3, O_: 2, F_: 1, SI_: 4, P_: 3, S_: 2, CL_: 1, BR_: 1, I_: 1}
GROW = [C_] * 10 + [N_] * 4 + [O_] * 4 + [S_, P_, F_, F_, CL_, BR_, I_, B_, SI_]
AROMATIC_RINGS = [([C_] * 6, 6), ([N_] + [C_] * 5, 6), ([N_, C_, N_, C_, C_, C_], 6), ([N_] + [C_] * 4, 5), ([O_] + [C_] * 4, 5), ([S_] + [C_] * 4, 5)]
DESIGNED = [
    ([C_], {}), ([O_], {}), ([N_], {}),                                                            # methane (h = 4), water, ammonia
    ([C_, F_, F_, F_, O_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1, (4, 5): 1}),            # a trifluoromethyl ether: nb_het 4, nb_hal 3
    ([S_, O_, O_, O_, N_, C_, C_], {(0, 1): 2, (0, 2): 2, (0, 3): 1, (0, 4): 1, (3, 5): 1, (4, 6): 1}),   # a sulfamate: nb_no 4
    ([C_, C_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1}),                           # neopentane: deg 4
    ([C_, C_, C_], {(0, 1): 2, (1, 2): 2}),                                                         # allene: n_dbl 2
    ([N_, C_, C_], cycle(3, 1)),                                                                    # aziridine
]


def random_graph(rng, n):
    """(classes, bonds) of n atoms: an aromatic ring or a lone atom, then atoms attached one by one to an atom with a free valence,
    by a single, double or triple bond as both allow; now and then a ring closure between two atoms with free valences."""
    classes, bonds, free = [], {}, []
    if n >= 7 and rng.random() < 0.7:
        ring, size = AROMATIC_RINGS[int(rng.integers(len(AROMATIC_RINGS)))]
        classes, bonds = list(ring), cycle(size, 4)
        # a ring atom keeps one valence for a substituent, except a pyridine-like N and the O / S of a five-ring
        free = [0 if (c == N_ and size == 6) or c in (O_, S_) else 1 for c in classes]
    else:
        classes, free = [C_], [4]
    while len(classes) < n:
        open_atoms = [i for i, f in enumerate(free) if f > 0]
        if not open_atoms:
            break
        a = int(rng.choice(open_atoms))
        el = int(rng.choice(GROW))
        if el == S_ and rng.random() < 0.5 and len(classes) + 3 <= n and free[a] >= 1:            # a sulfonyl group: S(=O)(=O)
            s = len(classes)
            classes += [S_, O_, O_]
            free += [1, 0, 0]
            bonds.update({(a, s): 1, (s, s + 1): 2, (s, s + 2): 2})
            free[a] -= 1
            continue
        order = int(rng.choice([1, 1, 1, 1, 2, 2, 3]))
        order = min(order, free[a], VALENCE[el])
        if a < len(classes) and any(bonds.get((min(a, z), max(a, z))) == 4 for z in range(len(classes)) if z != a):
            order = 1                                                                          # substituents of aromatic atoms are single-bonded
        b = len(classes)
        classes.append(el)
        free.append(VALENCE[el] - order)
        free[a] -= order
        bonds[(a, b)] = order
        if rng.random() < 0.15:                                                                  # a ring closure, three atoms and more
            others = [i for i, f in enumerate(free[:-1]) if f > 0 and i != a and (min(i, b), max(i, b)) not in bonds]
            if others and free[b] > 0:
                c = int(rng.choice(others))
                if not any(o == 4 for (x, y), o in bonds.items() if c in (x, y)):
                    bonds[(min(b, c), max(b, c))] = 1
                    free[b] -= 1
                    free[c] -= 1
    return classes, bonds


def random_family(seed=FAMILY_SEED, n_graphs=FAMILY_GRAPHS):
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.integers(2, FAMILY_MAX + 1, size=n_graphs)]
    return [random_graph(rng, n) for n in sizes] + [(list(c), dict(b)) for c, b in DESIGNED]


# ---- tools/props_host_check.cpp ---------------------------------------------------------------------------------------------------------
def write_cases(path, cases):
    """cases: [(rows of one graph as `cpu_inputs` gives them, tables, pairs, max_violations)].  Per case: a line `n n_rows n_tables
    max_violations kekule_status`; the n triples `cls hcount charge atom_ring`; n_rows quintuples `a b order kekule_order ring_size`;
    per table its row count and its rows; the nine limit pairs."""
    with open(path, 'w') as fh:
        for (cls, order, kek, h, q, status, ring_size, atom_ring), tables, pairs, max_violations in cases:
            n = len(cls)
            rows, a, b = MS.listed_pairs(n, order)
            fh.write('%d %d %d %d %d\n' % (n, len(rows), len(tables), max_violations, status))
            fh.write(' '.join('%d %d %d %d' % (cls[i], h[i], q[i], atom_ring[i]) for i in range(n)) + '\n')
            fh.write(' '.join('%d %d %d %d %d' % (x, y, order[r], kek[r], ring_size[r]) for x, y, r in zip(a, b, rows)) + '\n')
            for t in tables:
                fh.write('%d %s\n' % (len(t), ' '.join('%d %d %d %d' % tuple(r) for r in t)))
            fh.write(' '.join('%d %d' % p for p in pairs) + '\n')


def expected_lines(want, n_tables):
    """The three lines the program prints for a case, from the restatement's outputs."""
    n = len(want['atom_env'])
    return [' '.join(str(int(x)) for x in [want['status'], want['violated'], want['weight_milli'], *want['sums'], *want['counts']]),
            ' '.join(str(int(x)) for x in want['atom_env']),
            ' '.join(str(int(want['atom_row'][t, i])) for t in range(4) for i in range(n))]


def run_host_check(exe, cases, work_dir):
    path = os.path.join(str(work_dir), 'props_cases.txt')
    write_cases(path, cases)
    return MS.run_program(exe, path)
