"""Which kernel form a pg_seg_attn / pg_seg_attn_bwd call runs: the two resolvers (pg_seg_attn_form, pg_seg_attn_bwd_form) through
ctypes, without a GPU -- they are host arithmetic on the arguments, every pointer here is a dummy that nothing dereferences.  The rows
walk the boundaries of the dispatch (csrc/seg_form.hip); the limits' mirrors in phoregen_amd/hip.py are held against the header."""
import ctypes as C
import itertools
import re

import pytest

import mol_support as ms
from phoregen_amd import hip

OK, ERR_ARG = 0, 1
_dummy = (C.c_int * 256)()
P = (C.addressof(_dummy) + 15) // 16 * 16               # a non-NULL, 16-byte aligned pointer that nothing may dereference
KNN_NODE, KNN_POS, BOND_NODE, BOND_POS, TRIPLET, PHORE = range(6)
TWO_LISTS, FOLD_UNFOLD, SECOND_LAUNCH = hip.PG_FORM_TWO_LISTS, hip.PG_FORM_FOLD_UNFOLD, hip.PG_FORM_SECOND_LAUNCH


@pytest.fixture(autouse=True)
def _debug_word_off():
    lib = hip.load_library()
    old = lib.pg_debug_force_generic_seg(0)
    yield
    lib.pg_debug_force_generic_seg(old)


def topo(max_nlig=40):
    t = hip.PgTopo()
    t.max_nlig, t.n_lig = max_nlig, 100
    return t


def seg(mode, fused=False, **kw):
    s = hip.PgSegAttn()
    s.mode, s.n_seg, s.knn_k, s.seg_ids, s.U = mode, 7, 32, P, P
    s.Csrc_k, s.Csrc_v, s.ld_csrc, s.Cdst_k, s.Cdst_v, s.ld_cdst = P, P + 512, 256, P, P + 512, 256
    if mode in (KNN_POS, BOND_POS):
        s.dx = P
    else:
        s.S, s.swn = P, P
    if fused:
        s.q, s.W2k_l = P, P
        if mode in (KNN_NODE, BOND_NODE):
            s.W2v_l, s.b2v, s.out = P, P, P
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def fwd(t, s, force=0):
    """(rc, form) of pg_seg_attn_form under the debug word `force`."""
    lib, f = hip.load_library(), hip.PgSegForm()
    lib.pg_debug_force_generic_seg(force)
    rc = lib.pg_seg_attn_form(C.byref(t), C.byref(s), C.byref(f))
    lib.pg_debug_force_generic_seg(0)
    return rc, f


def fwd_ok(t, s, force=0):
    rc, f = fwd(t, s, force)
    assert rc == OK, hip.load_library().pg_last_error()
    return f


def what(f):
    return (f.family, f.tiles, f.threads, f.compose, f.record_floats)


# ---- the mirrors ----
def test_limits_and_form_names_mirror_the_header():
    for name in hip.SEG_LIMITS:
        assert ms.header_macro(name) is not None and int(ms.header_macro(name)) == getattr(hip, name), name
    enum = dict(re.findall(r'\b(PG_FORM_[A-Z_]+) = (\d+)', ms.header_text()))
    assert len(enum) == len(hip.FORM_NAMES) == 10
    for name, value in enum.items():
        assert getattr(hip, name[3:]) == int(value) and hip.FORM_NAMES[int(value)] == name[8:].lower(), name
    assert C.sizeof(hip.PgSegForm) == 9 * 4
    assert hip.ABI_VERSION == 11 == hip.load_library().pg_abi_version()


def test_form_names_tell_the_forms_apart():
    t = topo(49)
    names = {hip.form_name(fwd_ok(t, s, force)) for s, force in (
        (seg(BOND_POS), 0), (seg(BOND_POS, True), 0), (seg(BOND_POS, True, pos_tiled=1), 0), (seg(BOND_POS, True), 1),
        (seg(BOND_NODE, True), 1), (seg(BOND_NODE, alpha=P, alpha_rows=64), 0), (seg(KNN_NODE, n_seg2=3, seg_ids2=P, Wf_k2=P, Wf_v2=P), 0))}
    assert names == {'node_two_pass/t4/256', 'node_fused/t4/768', 'pos_tiled/t4/768', 'fold+generic/256', 'fold+generic/256+unfold',
                     'node_two_pass/t4/256/rec16', '2x node_two_pass/t2/256'}


# ---- forward ----
def test_nothing_to_do_and_unknown_modes():
    lib = hip.load_library()
    assert fwd_ok(topo(), seg(KNN_NODE, n_seg=0)).family == hip.FORM_NONE
    rc, _ = fwd(topo(), seg(6))
    assert rc == ERR_ARG and b'unknown mode 6' in lib.pg_last_error()
    assert lib.pg_seg_attn_form(None, C.byref(seg(0)), C.byref(hip.PgSegForm())) == ERR_ARG and b'null argument' in lib.pg_last_error()
    assert what(fwd_ok(topo(), seg(PHORE))) == (hip.FORM_GENERIC, 0, 256, 0, 0)
    assert what(fwd_ok(topo(), seg(PHORE, alpha=P, alpha_rows=16))) == (hip.FORM_GENERIC, 0, 256, 0, 16)
    # the entry point itself refuses the same way, before it touches the runtime
    assert lib.pg_seg_attn(C.byref(topo()), C.byref(seg(6)), None) == ERR_ARG and b'unknown mode 6' in lib.pg_last_error()


@pytest.mark.parametrize('mode', (KNN_NODE, KNN_POS))
def test_knn_modes_at_k_32_and_33(mode):
    lib, t = hip.load_library(), topo()
    pos = mode == KNN_POS
    rec = 32 if pos else 16
    assert what(fwd_ok(t, seg(mode))) == (hip.FORM_NODE_TWO_PASS, 2, 256, 0, 0)
    assert what(fwd_ok(t, seg(mode, alpha=P, alpha_rows=32))) == (hip.FORM_NODE_TWO_PASS, 2, 256, 0, rec)
    assert what(fwd_ok(t, seg(mode, True))) == (hip.FORM_NODE_FUSED, 2, 768, 0, 0)
    assert what(fwd_ok(t, seg(mode, True, alpha=P, alpha_rows=32))) == (hip.FORM_NODE_FUSED, 2, 768, 0, rec)
    assert what(fwd_ok(t, seg(mode, knn_k=33))) == (hip.FORM_GENERIC, 0, 256, 0, 0)
    assert what(fwd_ok(t, seg(mode, knn_k=33, alpha=P, alpha_rows=48))) == (hip.FORM_GENERIC, 0, 256, 0, 0)     # the generic kernel leaves no record
    assert what(fwd_ok(t, seg(mode), force=1)) == (hip.FORM_GENERIC, 0, 256, 0, 0)
    # a fused request where the one-pass kernel has to run: fold + one-pass + unfold through the caller's scratch
    assert what(fwd_ok(t, seg(mode, True, knn_k=33))) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD, 0)
    assert what(fwd_ok(t, seg(mode, True), force=1)) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD, 0)
    for missing in ('U', 'seg_ids') + (() if pos else ('S', 'swn')):
        rc, _ = fwd(t, seg(mode, True, knn_k=33, **{missing: None}))
        assert rc == ERR_ARG and b'scratch' in lib.pg_last_error(), missing
    # the weight tables go to LDS in 16-byte pieces (not asked of the forced generic kernel)
    for table in ('Wf_k', 'Wf_v', 'Wf_k2', 'Wf_v2', 'W2xv_l'):
        rc, _ = fwd(t, seg(mode, **{table: P + 4}))
        assert rc == ERR_ARG and b'16-byte aligned' in lib.pg_last_error(), table
        assert fwd(t, seg(mode, **{table: P + 4}), force=1)[0] == OK


@pytest.mark.parametrize('mode', (BOND_NODE, BOND_POS))
@pytest.mark.parametrize('fused', (False, True))
def test_bond_modes_by_row_tiles(mode, fused):
    family, threads = (hip.FORM_NODE_FUSED, 768) if fused else (hip.FORM_NODE_TWO_PASS, 256)
    for n, tiles in ((2, 3), (32, 3), (48, 3), (49, 4), (64, 4), (65, 5), (80, 5)):
        assert what(fwd_ok(topo(n), seg(mode, fused))) == (family, tiles, threads, 0, 0), n
    rec = 32 if mode == BOND_POS else 16
    assert what(fwd_ok(topo(80), seg(mode, fused, alpha=P, alpha_rows=80))) == (family, 5, threads, 0, rec)
    assert what(fwd_ok(topo(81), seg(mode, fused, alpha=P, alpha_rows=96))) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD if fused else 0, 0)
    assert what(fwd_ok(topo(48), seg(mode, fused), force=1)) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD if fused else 0, 0)


def test_tiled_position_form():
    tiled = lambda tiles: (hip.FORM_POS_TILED, tiles, 768, 0, 0)
    for n, tiles in ((5, 2), (32, 2), (33, 3), (48, 3), (49, 4), (64, 4)):
        assert what(fwd_ok(topo(n), seg(BOND_POS, True, pos_tiled=1))) == tiled(tiles), n
    assert what(fwd_ok(topo(65), seg(BOND_POS, True, pos_tiled=1))) == (hip.FORM_NODE_FUSED, 5, 768, 0, 0)
    assert what(fwd_ok(topo(81), seg(BOND_POS, True, pos_tiled=1))) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD, 0)
    assert what(fwd_ok(topo(), seg(KNN_POS, True, pos_tiled=1))) == tiled(2)
    assert what(fwd_ok(topo(), seg(KNN_POS, True, pos_tiled=1, knn_k=33))) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD, 0)
    # not tiled: training outputs, a second list, no fused request, a node-update mode, the forced generic kernel
    assert what(fwd_ok(topo(40), seg(BOND_POS, True, pos_tiled=1, alpha=P, alpha_rows=48))) == (hip.FORM_NODE_FUSED, 3, 768, 0, 32)
    assert what(fwd_ok(topo(), seg(KNN_POS, True, pos_tiled=1, n_seg2=3, seg_ids2=P, Wf_k2=P, Wf_v2=P))) == (hip.FORM_NODE_FUSED, 2, 768, 0, 0)
    assert what(fwd_ok(topo(40), seg(BOND_POS, pos_tiled=1))) == (hip.FORM_NODE_TWO_PASS, 3, 256, 0, 0)
    assert what(fwd_ok(topo(40), seg(BOND_NODE, True, pos_tiled=1))) == (hip.FORM_NODE_FUSED, 3, 768, 0, 0)
    assert what(fwd_ok(topo(40), seg(BOND_POS, True, pos_tiled=1), force=1)) == (hip.FORM_GENERIC, 0, 256, FOLD_UNFOLD, 0)


def test_two_target_lists():
    lib, t = hip.load_library(), topo()
    two = dict(n_seg2=3, seg_ids2=P, Wf_k2=P, Wf_v2=P)
    for mode in (KNN_NODE, KNN_POS):
        assert what(fwd_ok(t, seg(mode, True, **two))) == (hip.FORM_NODE_FUSED, 2, 768, 0, 0)               # one launch
        assert what(fwd_ok(t, seg(mode, **two))) == (hip.FORM_NODE_TWO_PASS, 2, 256, TWO_LISTS, 0)          # not fused: list after list
        assert what(fwd_ok(t, seg(mode, **two), force=1)) == (hip.FORM_GENERIC, 0, 256, TWO_LISTS, 0)
        assert what(fwd_ok(t, seg(mode, True, **two), force=1)) == (hip.FORM_GENERIC, 0, 256, TWO_LISTS | FOLD_UNFOLD, 0)
        assert what(fwd_ok(t, seg(mode, True, knn_k=33, **two))) == (hip.FORM_GENERIC, 0, 256, TWO_LISTS | FOLD_UNFOLD, 0)
        assert what(fwd_ok(t, seg(mode, True, n_seg=0, **two))) == (hip.FORM_NODE_FUSED, 2, 768, TWO_LISTS, 0)   # an empty first list
        for missing in ('seg_ids', 'seg_ids2', 'Wf_k2', 'Wf_v2'):
            rc, _ = fwd(t, seg(mode, True, **dict(two, **{missing: None})))
            assert rc == ERR_ARG and b'second target list' in lib.pg_last_error(), missing
    for mode in (BOND_NODE, BOND_POS, TRIPLET, PHORE):
        rc, _ = fwd(t, seg(mode, **two))
        assert rc == ERR_ARG and b'second target list needs a knn mode' in lib.pg_last_error(), mode


def staged(train=False, **kw):
    base = dict(tri_iters=P, n_tri_iters=9, tri_counter=P, q=P, W2k_l=P, W2v_l=P, b2v=P)
    base.update(dict(S=P, swn=P) if train else dict(S=None, swn=None, out=P, resid=P))
    base.update(kw)
    return seg(TRIPLET, **base)


def test_staged_triplet():
    generic = (hip.FORM_GENERIC, 0, 256, 0, 0)
    assert what(fwd_ok(topo(), staged())) == (hip.FORM_TRI_STAGED, 3, 768, 0, 0)
    assert what(fwd_ok(topo(), staged(True))) == (hip.FORM_TRI_STAGED_TRAIN, 3, 768, 0, 0)
    assert what(fwd_ok(topo(), staged(True, alpha=P, alpha_rows=40))) == (hip.FORM_TRI_STAGED_TRAIN, 3, 768, 0, 16)
    assert what(fwd_ok(topo(), seg(TRIPLET))) == generic
    for kw in (dict(tri_iters=None), dict(tri_counter=None), dict(n_tri_iters=0), dict(Csrc_v=P + 516), dict(ld_csrc=260), dict(Csrc_k=P + 4, Csrc_v=P + 516),
               dict(Cdst_k=None), dict(Cdst_v=None)):
        for train in (False, True):
            assert what(fwd_ok(topo(), staged(train, **kw))) == generic, kw
    for kw in (dict(alpha=P, alpha_rows=48), dict(out=None), dict(resid=None)):
        assert what(fwd_ok(topo(), staged(**kw))) == generic, kw
    for kw in (dict(swn=None), dict(q=None), dict(W2k_l=None), dict(alpha=P, alpha_rows=39)):
        assert what(fwd_ok(topo(), staged(True, **kw))) == generic, kw
    assert what(fwd_ok(topo(81), staged())) == (hip.FORM_TRI_STAGED, 5, 768, 0, 0) and what(fwd_ok(topo(82), staged())) == generic
    assert hip.PG_SEG_TRI_STAGED_ROWS + 1 == 81 < hip.PG_SEG_TRI_STAGED_ATOMS
    # the instance is the one for the largest ligand of the QUEUE: a segment visits n - 2 rows
    for train in (False, True):
        family = hip.FORM_TRI_STAGED_TRAIN if train else hip.FORM_TRI_STAGED
        for n, tiles in ((3, 3), (50, 3), (51, 4), (66, 4), (67, 5), (81, 5)):
            assert what(fwd_ok(topo(n), staged(train))) == (family, tiles, 768, 0, 0), n
            assert what(fwd_ok(topo(81), staged(train, tri_max_nlig=n))) == (family, tiles, 768, 0, 0), n
        assert fwd_ok(topo(50), staged(train, tri_max_nlig=70)).tiles == 3                  # (never above PgTopo.max_nlig)
    # debug bit 2: the sampling form on 8 waves; the training form has no such instance
    assert what(fwd_ok(topo(51), staged(), force=4)) == (hip.FORM_TRI_STAGED, 4, 512, 0, 0)
    assert what(fwd_ok(topo(51), staged(True), force=4)) == (hip.FORM_TRI_STAGED_TRAIN, 4, 768, 0, 0)
    assert what(fwd_ok(topo(51), staged(), force=1)) == (hip.FORM_TRI_STAGED, 4, 768, 0, 0)        # bit 0 is about the node modes


# ---- adjoint ----
def grad(record=False, scratch=False, rowbuf=True, **kw):
    g = hip.PgSegAttnGrad()
    g.grid, g.rowbuf_rows = 8, 96
    if record:
        g.alpha, g.alpha_rows, g.S, g.swn = P, 96, P, P
    if scratch:
        g.dlogit, g.gfeat_v = P, P
    if rowbuf:
        g.rowbuf = P
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def bwd(t, s, g):
    lib, f = hip.load_library(), hip.PgSegForm()
    return lib.pg_seg_attn_bwd_form(C.byref(t), C.byref(s), C.byref(g), C.byref(f)), f


def bwd_what(t, s, g):
    rc, f = bwd(t, s, g)
    assert rc == OK, hip.load_library().pg_last_error()
    return (f.family, f.threads, f.threads2, f.record_floats, f.rowbuf_waves)


def dispatch_before(mode, max_nlig, alpha, S_swn, scratch):
    """The adjoint's dispatch as pg_seg_attn_bwd had it before the resolver, restated from its switch: (family, threads of the first
    launch, threads of the second, floats per row read of the record, waves of the largest workgroup)."""
    op = alpha and S_swn
    one, two = hip.FORM_BWD_ONE_WAVE, hip.FORM_BWD_TWO_PASS
    if mode == KNN_NODE:
        return (two, 256, 256, 16, 4) if op and scratch else (one, 256, 0, 16 if op else 0, 4)
    if mode == KNN_POS:
        return (two, 256, 256, 32, 4) if alpha and scratch else (one, 256, 0, 0, 4)
    if mode in (BOND_NODE, PHORE):
        return (one, 256, 0, 16 if op else 0, 4)
    if mode == BOND_POS:
        return (one, 256, 0, 0, 4)
    if op and scratch and max_nlig <= 64:
        return (two, 512, 256, 16, 8)
    return (one, 256, 0, 16 if op else 0, 4) if max_nlig <= 64 else (one, 128, 0, 16 if op else 0, 2)


@pytest.mark.parametrize('mode', range(6))
def test_adjoint_forms_follow_the_pointers(mode):
    for max_nlig, alpha, S_swn, scratch in itertools.product((40, 64, 65, 80), (False, True), (False, True), (False, True)):
        g = grad(scratch=scratch, alpha=P if alpha else None, S=P if S_swn else None, swn=P if S_swn else None)
        assert bwd_what(topo(max_nlig), seg(mode), g) == dispatch_before(mode, max_nlig, alpha, S_swn, scratch), (max_nlig, alpha, S_swn, scratch)
    # one of S / swn alone is no record (the knn position update reads logits | value scalars and neither of the two)
    assert bwd_what(topo(), seg(mode), grad(True, True, swn=None))[0] == (hip.FORM_BWD_TWO_PASS if mode == KNN_POS else hip.FORM_BWD_ONE_WAVE)
    assert hip.load_library().pg_seg_attn_bwd_waves(mode) == (8 if mode == TRIPLET else 4)


def test_adjoint_triplet_waves_and_the_two_pass_limit():
    assert bwd_what(topo(64), seg(TRIPLET), grad(True)) == (hip.FORM_BWD_ONE_WAVE, 256, 0, 16, 4)
    assert bwd_what(topo(65), seg(TRIPLET), grad(True)) == (hip.FORM_BWD_ONE_WAVE, 128, 0, 16, 2)
    assert bwd_what(topo(64), seg(TRIPLET), grad(True, True)) == (hip.FORM_BWD_TWO_PASS, 512, 256, 16, 8)
    assert bwd_what(topo(65), seg(TRIPLET), grad(True, True)) == (hip.FORM_BWD_ONE_WAVE, 128, 0, 16, 2)      # two passes up to 64 atoms only


def test_adjoint_channel_split():
    split = lambda n, form, **kw: bwd(topo(n), seg(TRIPLET, **kw), grad(True, True, rowbuf=False, tri_form=form))
    for n, nt in ((5, 2), (32, 2), (33, 3), (48, 3), (49, 4), (64, 4)):
        rc, f = split(n, 1)
        assert rc == OK and (f.family, f.tiles, f.threads, f.compose, f.threads2, f.rowbuf_waves) == (hip.FORM_BWD_CHANNEL_SPLIT, nt, 256, 0, 0, 0), n
        rc, f = split(n, 2)
        assert rc == OK and (f.family, f.tiles, f.threads, f.rowbuf_waves, f.record_floats) == (hip.FORM_BWD_CHANNEL_SPLIT, 2, 512, 0, 0), n
        assert (f.compose, f.tiles2, f.threads2) == ((SECOND_LAUNCH, nt, 256) if nt > 2 else (0, 0, 0)), n
    # above 64 atoms, or with Cdst_k / Cdst_v not the halves of one row: the one-wave form (which needs the row buffer)
    lib = hip.load_library()
    for form in (1, 2):
        rc, _ = split(65, form)
        assert rc == ERR_ARG and b'rowbuf' in lib.pg_last_error()
        rc, _ = split(40, form, Cdst_v=P + 1024)
        assert rc == ERR_ARG and b'rowbuf' in lib.pg_last_error()
        assert bwd_what(topo(40), seg(TRIPLET, Cdst_v=P + 1024), grad(True, tri_form=form)) == (hip.FORM_BWD_ONE_WAVE, 256, 0, 16, 4)
        assert bwd_what(topo(65), seg(TRIPLET), grad(True, tri_form=form)) == (hip.FORM_BWD_ONE_WAVE, 128, 0, 16, 2)
        assert bwd_what(topo(40), seg(BOND_NODE), grad(True, tri_form=form)) == (hip.FORM_BWD_ONE_WAVE, 256, 0, 16, 4)   # a triplet switch only


def test_adjoint_refusals():
    lib = hip.load_library()
    for mode, record, scratch in itertools.product(range(6), (False, True), (False, True)):
        rc, _ = bwd(topo(), seg(mode), grad(record, scratch, rowbuf=False))
        assert rc == ERR_ARG and b'needs PgSegAttnGrad.rowbuf' in lib.pg_last_error(), mode
    for kw in (dict(U=None), dict(Cdst_k=None), dict(Cdst_v=None)):
        assert bwd(topo(), seg(KNN_NODE, **kw), grad())[0] == ERR_ARG and b'are required' in lib.pg_last_error()
    assert bwd(topo(), seg(KNN_NODE), grad(grid=0))[0] == ERR_ARG and b'are required' in lib.pg_last_error()
    assert bwd(topo(), seg(7), grad())[0] == ERR_ARG and b'unknown mode 7' in lib.pg_last_error()
    rc, f = bwd(topo(), seg(TRIPLET, n_seg=0), grad(rowbuf=False))
    assert rc == OK and f.family == hip.FORM_NONE
    assert lib.pg_seg_attn_bwd(C.byref(topo()), C.byref(seg(KNN_NODE)), C.byref(grad(rowbuf=False)), None) == ERR_ARG      # the entry point, before any launch
    assert b'needs PgSegAttnGrad.rowbuf' in lib.pg_last_error()


def test_adjoint_refuses_the_first_ligand_whose_rows_do_not_fit_the_lds():
    """The triplet's one-wave form on 2 waves: base + 2 waves + a row of 259 floats per atom of max_nlig rounded up to a row tile."""
    lib = hip.load_library()
    base, wave, row, budget, tile = (hip.PG_SEG_BWD_TRI_BASE_FLOATS, hip.PG_SEG_BWD_TRI_WAVE_FLOATS, hip.PG_SEG_BWD_TRI_ROW_FLOATS,
                                     hip.PG_SEG_BWD_LDS_BYTES, hip.PG_SEG_ROW_TILE)
    need = lambda n, waves: 4 * (base + waves * wave + -(-n // tile) * tile * row)
    assert need(hip.PG_SEG_BWD_TRI_MAX_ATOMS, 4) <= budget                     # the 4-wave form holds every ligand it is chosen for
    first = next(n for n in range(hip.PG_SEG_BWD_TRI_MAX_ATOMS + 1, 1000) if need(n, 2) > budget)
    assert first > hip.PG_SEG_TRI_STAGED_ATOMS                                 # (whatever the forward kernels hold has an adjoint)
    for record in (False, True):
        assert bwd(topo(first - 1), seg(TRIPLET), grad(record))[0] == OK
        rc, _ = bwd(topo(first), seg(TRIPLET), grad(record))
        assert rc == ERR_ARG and lib.pg_last_error() == b'pg_seg_attn_bwd: %d B of LDS needed (ligand of %d atoms is too large)' % (need(first, 2), first)
    assert bwd(topo(first), seg(BOND_NODE), grad())[0] == OK                   # arithmetic on max_nlig for the triplet only
