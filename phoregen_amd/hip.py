"""ctypes binding of libphoregen_hip.so (the C ABI declared in include/phoregen_hip.h).

There is NO fallback: if the library is missing or no GPU is visible the product path raises.
"""
import ctypes as C
import struct
import sys
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, '_lib', 'libphoregen_hip.so')

c_fp = C.c_void_p
c_ip = C.c_void_p


class PgGemm(C.Structure):
    _fields_ = [('X', c_fp), ('ldx', C.c_int), ('K1', C.c_int),
                ('X2', c_fp), ('ldx2', C.c_int), ('K2', C.c_int),
                ('W', c_fp), ('ldw', C.c_int),
                ('bias', c_fp),
                ('ln_gamma', c_fp), ('ln_beta', c_fp),
                ('add1', c_fp), ('ld_add1', C.c_int), ('idx1', c_ip),
                ('add2', c_fp), ('ld_add2', C.c_int), ('idx2', c_ip),
                ('out_scale', C.c_float), ('act', C.c_int),
                ('Y', c_fp), ('ldy', C.c_int), ('M', C.c_int), ('N', C.c_int), ('rows', c_ip), ('add_rows', C.c_int),
                ('row_extent', C.c_int), ('tile_rows', c_ip)]


class PgTopo(C.Structure):
    _fields_ = [('n_graphs', C.c_int), ('n_ctx', C.c_int), ('n_lig', C.c_int), ('n_phore', C.c_int),
                ('n_bond', C.c_int), ('max_nlig', C.c_int), ('max_gctx', C.c_int),
                ('g_ctx_off', c_ip), ('g_nph', c_ip), ('g_nlig', c_ip), ('g_eid_off', c_ip), ('eid', c_ip),
                ('ctx_graph', c_ip), ('ctx_is_lig', c_ip), ('lig2ctx', c_ip), ('bond_src', c_ip),
                ('bond_dst', c_ip), ('bond_desc', c_ip), ('g_bond_off', c_ip), ('edge_ref', c_ip)]


class PgSegAttn(C.Structure):
    _fields_ = [('mode', C.c_int), ('n_seg', C.c_int), ('seg_ids', c_ip), ('seg_chunks', c_ip),
                ('x', c_fp), ('nrm', c_fp), ('nbr', c_ip), ('deg', c_ip), ('ew', c_fp), ('knn_k', C.c_int),
                ('Csrc_k', c_fp), ('Csrc_v', c_fp), ('ld_csrc', C.c_int),
                ('Cdst_k', c_fp), ('Cdst_v', c_fp), ('ld_cdst', C.c_int),
                ('Wf_k', c_fp), ('Wf_v', c_fp), ('Wg2_k', c_fp), ('Wg2_v', c_fp), ('G', c_fp),
                ('ln_gk', c_fp), ('ln_bk', c_fp), ('ln_gv', c_fp), ('ln_bv', c_fp),
                ('U', c_fp), ('q', c_fp), ('W2k_l', c_fp), ('W2v_l', c_fp), ('b2v', c_fp),
                ('W2xv_l', c_fp), ('b2xv', c_fp),
                ('S', c_fp), ('swn', c_fp), ('resid', c_fp), ('out', c_fp), ('dx', c_fp),
                ('accumulate_dx', C.c_int), ('alpha', c_fp), ('alpha_rows', C.c_int), ('efeat', c_fp), ('efeat_off', c_ip),
                ('tri_iters', c_ip), ('n_tri_iters', C.c_int), ('tri_counter', c_ip),
                ('seg_ids2', c_ip), ('n_seg2', C.c_int), ('Wf_k2', c_fp), ('Wf_v2', c_fp), ('tri_grid', C.c_int), ('pos_tiled', C.c_int), ('tri_max_nlig', C.c_int)]


class PgSegAttnGrad(C.Structure):
    _fields_ = [('gS', c_fp), ('gswn', c_fp), ('gdx', c_fp), ('gU', c_fp),
                ('gCdst_k', c_fp), ('gCdst_v', c_fp), ('ld_gcdst', C.c_int),
                ('gCsrc_k', c_fp), ('gCsrc_v', c_fp), ('ld_gcsrc', C.c_int),
                ('gWf_k', c_fp), ('gWf_v', c_fp), ('gbk', c_fp), ('gbv', c_fp),
                ('gW2xv_l', c_fp), ('gb2xv', c_fp), ('gx', c_fp), ('gnrm', c_fp), ('gew', c_fp),
                ('alpha', c_fp), ('alpha_rows', C.c_int), ('S', c_fp), ('swn', c_fp),
                ('rowbuf', c_fp), ('rowbuf_rows', C.c_int), ('grid', C.c_int), ('atom_order', c_ip),
                ('dlogit', c_fp), ('gfeat_v', c_fp), ('tri_form', C.c_int)]


class PgSegForm(C.Structure):
    """What a pg_seg_attn / pg_seg_attn_bwd call runs (pg_seg_attn_form / pg_seg_attn_bwd_form)."""
    _fields_ = [('mode', C.c_int), ('family', C.c_int), ('tiles', C.c_int), ('threads', C.c_int), ('compose', C.c_int),
                ('tiles2', C.c_int), ('threads2', C.c_int), ('record_floats', C.c_int), ('rowbuf_waves', C.c_int)]

    def key(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


PG_PROGRAM_LANES, PG_LAUNCH_MAX_ARGS = 4, 12


class PgLaunch(C.Structure):
    _fields_ = [('op', C.c_int32), ('lane', C.c_int32), ('ev', C.c_int32), ('n_arg', C.c_int32), ('a', C.c_uint64 * PG_LAUNCH_MAX_ARGS)]


OP_RECORD, OP_WAIT = 0, 1
# entry point -> PG_OP_* (include/phoregen_hip.h): what a launch list handed to pg_program_create may hold
PROGRAM_OPS = {'pg_gemm': 2, 'pg_seg_attn': 3, 'pg_embed_ctx': 4, 'pg_embed_bond': 5, 'pg_knn_ctx': 6, 'pg_lig_normals': 7,
               'pg_edge_gate': 8, 'pg_knn_group_by_kind': 9, 'pg_bond_smear': 10, 'pg_attn_fold_query': 11,
               'pg_attn_unfold_value': 12, 'pg_apply_dx': 13, 'pg_layer_geom': 14, 'pg_rows_linear': 15, 'pg_atom_count': 16,
               'pg_embed_bond_e16': 17}

SEG_KNN_NODE, SEG_KNN_POS, SEG_BOND_NODE, SEG_BOND_POS, SEG_TRIPLET, SEG_PHORE = range(6)
ACT_NONE, ACT_SSP, ACT_RELU = 0, 1, 2

# kernel families and composite cases of a PgSegForm, and the limits of the forms, as the PG_FORM_* / PG_SEG_* macros of the header
(FORM_NONE, FORM_GENERIC, FORM_NODE_TWO_PASS, FORM_NODE_FUSED, FORM_POS_TILED, FORM_TRI_STAGED, FORM_TRI_STAGED_TRAIN,
 FORM_BWD_ONE_WAVE, FORM_BWD_TWO_PASS, FORM_BWD_CHANNEL_SPLIT) = range(10)
FORM_NAMES = ('none', 'generic', 'node_two_pass', 'node_fused', 'pos_tiled', 'tri_staged', 'tri_staged_train',
              'bwd_one_wave', 'bwd_two_pass', 'bwd_channel_split')
PG_FORM_TWO_LISTS, PG_FORM_FOLD_UNFOLD, PG_FORM_SECOND_LAUNCH = 1, 2, 4
PG_SEG_ROW_TILE, PG_SEG_KNN_MAX_K = 16, 32
PG_SEG_NODE_MIN_TILES, PG_SEG_NODE_MAX_TILES, PG_SEG_POS_TILED_MIN_TILES, PG_SEG_POS_TILED_MAX_TILES = 3, 5, 2, 4
PG_SEG_TRI_STAGED_ROWS, PG_SEG_TRI_STAGED_ATOMS, PG_SEG_TRI_STAGED_LD = 80, 96, 256
PG_SEG_TRI_MIN_TILES, PG_SEG_TRI_MAX_TILES, PG_SEG_TRI_WAVES, PG_SEG_TRI_WAVES_DEBUG = 3, 5, 12, 8
PG_SEG_BWD_TRI_MAX_ATOMS, PG_SEG_BWD_TRI_FORM2_ATOMS = 64, 32
PG_SEG_BWD_LDS_BYTES, PG_SEG_BWD_TRI_BASE_FLOATS, PG_SEG_BWD_TRI_WAVE_FLOATS, PG_SEG_BWD_TRI_ROW_FLOATS = 163840, 7680, 3072, 259
PG_SEG_PHORE_RECORD_ROWS = 256
SEG_LIMITS = ('PG_SEG_ROW_TILE', 'PG_SEG_KNN_MAX_K', 'PG_SEG_NODE_MIN_TILES', 'PG_SEG_NODE_MAX_TILES', 'PG_SEG_POS_TILED_MIN_TILES',
              'PG_SEG_POS_TILED_MAX_TILES', 'PG_SEG_TRI_STAGED_ROWS', 'PG_SEG_TRI_STAGED_ATOMS', 'PG_SEG_TRI_STAGED_LD',
              'PG_SEG_TRI_MIN_TILES', 'PG_SEG_TRI_MAX_TILES', 'PG_SEG_TRI_WAVES', 'PG_SEG_TRI_WAVES_DEBUG', 'PG_SEG_BWD_TRI_MAX_ATOMS',
              'PG_SEG_BWD_TRI_FORM2_ATOMS', 'PG_SEG_BWD_LDS_BYTES', 'PG_SEG_BWD_TRI_BASE_FLOATS', 'PG_SEG_BWD_TRI_WAVE_FLOATS',
              'PG_SEG_BWD_TRI_ROW_FLOATS', 'PG_SEG_PHORE_RECORD_ROWS', 'PG_FORM_TWO_LISTS', 'PG_FORM_FOLD_UNFOLD', 'PG_FORM_SECOND_LAUNCH')

ABI_VERSION = 11
PG_MOL_MAX_ATOMS = 128          # include/phoregen_hip.h (the library refuses a larger graph before it launches anything)
# the substructure search (pg_mol_sub): the limits and the layout of a pattern row, as the PG_SUB_* macros of include/phoregen_hip.h
PG_SUB_MAX_ATOMS, PG_SUB_MAX_PATTERNS, PG_SUB_MAX_STEPS, PG_SUB_PATTERN_BYTES = 16, 256, 1 << 30, 416
PG_SUB_OFF_K, PG_SUB_OFF_MIN, PG_SUB_OFF_MAX, PG_SUB_OFF_ORDER, PG_SUB_OFF_ATOMS, PG_SUB_OFF_BONDS = 0, 4, 8, 16, 32, 160
PG_SUB_ATOM_BYTES, PG_SUB_ATOM_ELEMENTS, PG_SUB_ATOM_DEGREE, PG_SUB_ATOM_HCOUNT, PG_SUB_ATOM_FLAGS = 8, 0, 2, 4, 6
PG_SUB_ANY, PG_SUB_YES, PG_SUB_NO = 0, 1, 2
# the hydrogen placement (pg_mol_hydrogens): slots per atom, count columns and the degeneracy threshold, as the PG_HYD_* macros
PG_HYD_MAX_PER_ATOM, PG_HYD_N_COUNTS, PG_HYD_DEG_EPS = 4, 8, 1e-3
# the scaffold (pg_mol_scaffold): the flag bits, the values of `part`, carbon's class and the count columns, as the PG_SCAF_* macros
PG_SCAF_EXOCYCLIC, PG_SCAF_GENERIC, PG_SCAF_CARBON, PG_SCAF_N_COUNTS = 1, 2, 1, 8
PG_SCAF_PART_NONE, PG_SCAF_PART_SIDE_CHAIN, PG_SCAF_PART_LINKER, PG_SCAF_PART_RING, PG_SCAF_PART_EXOCYCLIC = range(5)
# the property descriptors (pg_mol_props): the limits of the tables, the status bits, the shift of every field of the environment word,
# the count columns and the limited quantities, as the PG_PROP_* macros
PG_PROP_MAX_ROWS, PG_PROP_MAX_TABLES, PG_PROP_ROW_INTS, PG_PROP_N_WEIGHTS = 128, 4, 4, 12
PG_PROP_NO_KEKULE, PG_PROP_LIMITS, PG_PROP_UNTYPED = 1, 2, 4
(PG_PROP_ENV_EL, PG_PROP_ENV_H, PG_PROP_ENV_Q, PG_PROP_ENV_DEG, PG_PROP_ENV_AROM, PG_PROP_ENV_N_DBL, PG_PROP_ENV_TRIPLE, PG_PROP_ENV_RING,
 PG_PROP_ENV_RING3, PG_PROP_ENV_NB_HET, PG_PROP_ENV_NB_AROM, PG_PROP_ENV_DBL_O, PG_PROP_ENV_DBL_HET, PG_PROP_ENV_NB_DBL_HET,
 PG_PROP_ENV_NB_HAL, PG_PROP_ENV_NB_NO) = 0, 4, 7, 8, 11, 12, 14, 15, 16, 17, 20, 22, 23, 24, 25, 27
(PG_PROP_C_HEAVY_ATOMS, PG_PROP_C_HYDROGENS, PG_PROP_C_CARBONS, PG_PROP_C_SP3_CARBONS, PG_PROP_C_HETEROATOMS, PG_PROP_C_HALOGENS,
 PG_PROP_C_NHOH, PG_PROP_C_NO_COUNT, PG_PROP_C_ROTATABLE, PG_PROP_C_AMIDE_BONDS, PG_PROP_C_AROMATIC_ATOMS, PG_PROP_C_RING_ATOMS,
 PG_PROP_C_NET_CHARGE, PG_PROP_C_UNTYPED, PG_PROP_C_VIOLATIONS) = range(15)
PG_PROP_N_COUNTS = 16
# the shape overlap (pg_shape_*): the length of the alpha table, the status bits and the tiles, as the PG_SHAPE_* macros
PG_SHAPE_N_ALPHA, PG_SHAPE_EMPTY, PG_SHAPE_NONFINITE, PG_SHAPE_UNSELECTED, PG_SHAPE_TILE_A, PG_SHAPE_TILE_B = 12, 1, 2, 4, 16, 16
# the overlay (pg_shape_frames, pg_shape_align): the floats of a frame, the starts and the bits of their mask, the largest max_steps
PG_SHAPE_FRAME_FLOATS, PG_SHAPE_ALIGN_N_STARTS, PG_SHAPE_ALIGN_IN_PLACE, PG_SHAPE_ALIGN_INERTIAL, PG_SHAPE_ALIGN_MAX_STEPS = 16, 5, 0x01, 0x1e, 1024
PG_PROP_L_WEIGHT, PG_PROP_L_HEAVY_ATOMS, PG_PROP_L_NHOH, PG_PROP_L_NO_COUNT, PG_PROP_L_ROTATABLE, PG_PROP_L_SUM0, PG_PROP_N_LIMITS = 0, 1, 2, 3, 4, 5, 9
_lib = None

_PROTOS = {
    'pg_last_error': (C.c_char_p, []),
    'pg_abi_version': (C.c_int, []),
    'pg_abi_struct_sizes': (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    'pg_order_point_create': (C.c_int, [C.POINTER(C.c_void_p)]),
    'pg_order_point_destroy': (C.c_int, [C.c_void_p]),
    'pg_order_point_record': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pg_order_point_wait': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pg_debug_order_point_fence_free': (C.c_int, [C.c_int]),
    'pg_program_create': (C.c_int, [C.POINTER(PgLaunch), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'pg_program_run': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    'pg_program_length': (C.c_int, [C.c_void_p]),
    'pg_program_destroy': (C.c_int, [C.c_void_p]),
    'pg_micro_mfma_f32': (C.c_int, [C.c_int, C.c_int, c_fp, C.POINTER(C.c_double), C.c_void_p]),
    'pg_selftest_mfma': (C.c_int, [c_ip, C.c_void_p]),
    'pg_selftest_philox': (C.c_int, [c_ip, C.c_int, c_ip, C.c_void_p]),
    'pg_debug_force_generic_seg': (C.c_int, [C.c_int]),
    'pg_gemm': (C.c_int, [C.POINTER(PgGemm), C.c_void_p]),
    'pg_debug_gemm_streaming': (C.c_int, [C.c_int]),
    'pg_gemm_is_streaming': (C.c_int, [C.POINTER(PgGemm)]),
    'pg_embed_ctx': (C.c_int, [C.POINTER(PgTopo)] + [c_fp] * 11 + [C.c_void_p]),
    'pg_embed_bond': (C.c_int, [C.POINTER(PgTopo)] + [c_fp] * 7 + [C.c_void_p]),
    'pg_embed_bond_e16': (C.c_int, [C.POINTER(PgTopo)] + [c_fp] * 8 + [C.c_void_p]),
    'pg_knn_ctx': (C.c_int, [C.POINTER(PgTopo), c_fp, C.c_int, c_ip, c_ip, C.c_void_p]),
    'pg_lig_normals': (C.c_int, [C.POINTER(PgTopo), c_fp, c_fp, c_ip, c_fp, C.c_void_p]),
    'pg_lig_nn3': (C.c_int, [C.POINTER(PgTopo), c_fp, c_ip, C.c_void_p]),
    'pg_edge_gate': (C.c_int, [C.POINTER(PgTopo), c_fp, c_ip, c_ip, C.c_int, c_fp, c_fp, c_fp, c_fp, c_fp,
                               C.c_float, c_fp, C.c_void_p]),
    'pg_knn_group_by_kind': (C.c_int, [C.POINTER(PgTopo), C.c_int, c_ip, c_ip, c_fp, C.c_void_p]),
    'pg_bond_smear': (C.c_int, [C.POINTER(PgTopo), c_fp, c_fp, C.c_void_p]),
    'pg_seg_attn': (C.c_int, [C.POINTER(PgTopo), C.POINTER(PgSegAttn), C.c_void_p]),
    'pg_seg_attn_form': (C.c_int, [C.POINTER(PgTopo), C.POINTER(PgSegAttn), C.POINTER(PgSegForm)]),
    'pg_attn_fold_query': (C.c_int, [c_fp, C.c_int, c_fp, C.c_int, c_ip, c_fp, C.c_void_p]),
    'pg_attn_unfold_value': (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int, c_ip, c_fp, C.c_int, C.c_void_p]),
    'pg_apply_dx': (C.c_int, [C.POINTER(PgTopo), c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_layer_geom': (C.c_int, [C.POINTER(PgTopo), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_attn_unfold_bias_grad': (C.c_int, [c_fp, C.c_int, c_fp, c_fp, C.c_int, c_ip, c_fp, c_fp, C.c_void_p]),
    'pg_bond_rows_sum': (C.c_int, [C.POINTER(PgTopo), c_fp, C.c_int, C.c_int, C.c_int, c_fp, C.c_int, C.c_void_p]),
    'pg_rows_linear': (C.c_int, [c_fp, C.c_int, C.c_int, c_fp, c_fp, C.c_int, C.c_int, c_ip, c_fp, C.c_int,
                                 C.c_void_p]),
    'pg_atom_count': (C.c_int, [c_fp, c_fp, c_ip, c_ip, C.c_int, C.c_int, c_fp, c_fp, C.c_void_p]),
    'pg_posterior_categorical': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_fp, c_fp, C.c_int, C.c_int, c_fp,
                                           C.c_uint64, C.c_uint32, C.c_uint32, c_ip, c_ip, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_posterior_position': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_uint64,
                                        C.c_uint32, C.c_uint32, C.c_int, c_ip, c_ip, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_posterior_position_ctx': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_uint64,
                                            C.c_uint32, C.c_uint32, C.c_int, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_posterior_categorical_frag': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_fp, c_fp, C.c_int, C.c_int, c_fp, C.c_uint64,
                                                C.c_uint32, C.c_uint32, c_ip, c_ip, c_fp, c_fp, c_fp, c_ip, C.c_uint32,
                                                C.c_void_p]),
    'pg_posterior_position_frag': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_uint64, C.c_uint32,
                                             C.c_uint32, C.c_int, c_ip, c_ip, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp,
                                             C.c_uint32, C.c_void_p]),
    'pg_posterior_position_ctx_frag': (C.c_int, [c_fp, c_fp, c_ip, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_uint64,
                                                 C.c_uint32, C.c_uint32, C.c_int, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip,
                                                 c_fp, c_fp, c_fp, C.c_uint32, C.c_void_p]),
    'pg_fragment_noise': (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.c_int, c_ip, c_ip, c_fp, c_ip, c_ip, c_ip, c_ip, c_ip,
                                    c_fp, c_fp, c_fp, c_fp, C.c_uint32, C.c_uint32, C.c_uint32, c_fp, c_fp, c_fp, c_fp, c_fp,
                                    C.c_void_p]),
    'pg_gemm_wgrad': (C.c_int, [c_fp, C.c_int, c_fp, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, C.c_int, c_fp, C.c_void_p]),
    'pg_ln_relu': (C.c_int, [c_fp, C.c_int, c_fp, c_fp, C.c_int, c_fp, C.c_int, C.c_void_p]),
    'pg_ln_relu_bwd': (C.c_int, [c_fp, C.c_int, c_fp, c_fp, c_fp, C.c_int, C.c_int, c_fp, C.c_int, c_fp, c_fp,
                                 C.c_void_p]),
    'pg_seg_attn_bwd_waves': (C.c_int, [C.c_int]),
    'pg_seg_attn_bwd': (C.c_int, [C.POINTER(PgTopo), C.POINTER(PgSegAttn), C.POINTER(PgSegAttnGrad), C.c_void_p]),
    'pg_seg_attn_bwd_form': (C.c_int, [C.POINTER(PgTopo), C.POINTER(PgSegAttn), C.POINTER(PgSegAttnGrad), C.POINTER(PgSegForm)]),
    'pg_attn_fold_wgrad': (C.c_int, [c_fp, C.c_int, c_fp, C.c_int, c_ip, c_fp, C.c_void_p]),
    'pg_guidance_grad': (C.c_int, [C.POINTER(PgTopo), c_fp, c_fp, c_ip, c_ip, C.c_int, C.c_float, C.c_float,
                                   C.c_int, c_fp, C.c_int, c_fp, c_fp, c_fp, C.c_void_p]),
    'pg_mol_screen': (C.c_int, [c_fp, C.c_int64, c_fp, C.c_int64, c_fp, C.c_int64, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_screen_dist': (C.c_int, [c_fp, C.c_int64, c_fp, C.c_int64, c_fp, C.c_int64, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, c_ip, c_fp, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_key': (C.c_int, [c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, c_ip, C.c_void_p]),
    'pg_mol_geom': (C.c_int, [c_fp, C.c_int64, c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_ip, C.c_int,
                              c_ip, c_ip, C.c_int, C.POINTER(C.c_float), c_fp, c_ip, c_fp, c_ip, c_ip, C.c_void_p]),
    'pg_mol_rings': (C.c_int, [c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), c_ip, c_ip, c_ip,
                               c_ip, c_ip, C.c_void_p]),
    'pg_mol_kekule': (C.c_int, [c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_ip, C.c_int, c_ip,
                                c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_feat': (C.c_int, [c_fp, C.c_int64, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_int, c_fp, c_ip, C.c_int, c_ip, c_ip, C.c_int, C.c_float, C.c_int, c_ip, c_fp, c_ip, c_ip,
                              c_ip, C.c_void_p]),
    'pg_mol_smiles': (C.c_int, [c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, C.c_int, c_ip,
                                c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_stereo': (C.c_int, [c_fp, C.c_int64, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_smiles_stereo': (C.c_int, [c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip,
                                       C.c_int, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_void_p]),
    'pg_mol_fp': (C.c_int, [c_ip, c_ip, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, c_ip, C.c_void_p]),
    'pg_fp_tanimoto': (C.c_int, [c_ip, C.c_int, c_ip, C.c_int, c_fp, C.c_void_p]),
    'pg_fp_nearest': (C.c_int, [c_ip, C.c_int, c_ip, C.c_int, C.c_int, c_fp, c_ip, c_fp, C.c_void_p]),
    'pg_fp_maxmin': (C.c_int, [c_ip, C.c_int, C.c_int, C.c_int, c_ip, c_fp, c_fp, c_ip, C.c_void_p]),
    'pg_mol_sub': (C.c_int, [c_ip] * 10 + [C.c_int] * 5 + [c_ip, c_ip, C.c_int, C.c_int] + [c_ip] * 5 + [C.c_void_p]),
    'pg_mol_hydrogens': (C.c_int, [c_fp, C.c_int64] + [c_ip] * 8 + [C.c_int] * 5 + [c_fp, C.c_float, C.c_int, c_fp, c_ip, c_ip, c_fp, c_ip, c_ip,
                                   C.c_void_p]),
    'pg_mol_scaffold': (C.c_int, [c_ip] * 4 + [C.c_int] * 6 + [c_ip] * 9 + [C.c_void_p]),
    'pg_mol_props': (C.c_int, [c_ip] * 10 + [C.c_int] * 5 + [c_ip, C.POINTER(C.c_int), C.c_int, c_ip, C.POINTER(C.c_int), C.c_int] + [c_ip] * 7
                     + [C.c_void_p]),
    'pg_shape_pack': (C.c_int, [c_ip, c_ip, c_fp, C.c_int64, c_ip, c_ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), c_fp, c_ip,
                                c_ip, C.c_void_p]),
    'pg_shape_self': (C.c_int, [c_fp, C.c_int, c_ip, C.c_int, C.POINTER(C.c_float), c_fp, c_fp, C.c_void_p]),
    'pg_shape_similarity': (C.c_int, [c_fp, C.c_int, c_ip, c_fp, c_fp, C.c_int] * 2 + [C.POINTER(C.c_float), c_fp, c_fp, C.c_void_p]),
    'pg_shape_nearest': (C.c_int, [c_fp, C.c_int, c_ip, c_fp, c_fp, C.c_int] * 2 + [C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), c_fp, c_ip,
                                   c_fp, C.c_void_p]),
    'pg_shape_frames': (C.c_int, [c_fp, C.c_int, c_ip, C.c_int, c_fp, C.c_void_p]),
    'pg_shape_align': (C.c_int, [c_fp, C.c_int, c_ip, c_fp, c_fp, c_fp, C.c_int] * 2 + [c_ip, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float),
                                 C.c_int, C.c_float, C.c_float, C.c_int, c_fp, c_fp, c_ip, c_ip, C.c_void_p]),
}

EXPORTS = tuple(_PROTOS)


def load_library(path=None):
    """Load the shared library and declare every prototype (no GPU needed for this)."""
    global _lib
    if _lib is not None:
        return _lib
    if path is None and os.environ.get('PHOREGEN_DEBUG') == '1':      # an instrumented / ablation build (tools/): only on explicit request
        path = os.environ.get('PHOREGEN_HIP_LIB')
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f'phoregen_amd: HIP extension not built: {path} is missing. '
                           f'Run `python -c "import __graft_entry__ as g; g.build()"` (hipcc, gfx950). '
                           f'There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    # the mirrors above against the build that was loaded: a stale .so (or a header edited without its mirror) fails here, not in a kernel
    if lib.pg_abi_version() != ABI_VERSION:
        raise RuntimeError(f'phoregen_amd: {path} has ABI version {lib.pg_abi_version()}, this package binds version {ABI_VERSION}: rebuild it')
    sizes = (C.c_int * 5)()
    lib.pg_abi_struct_sizes(sizes, 5)
    mine = [C.sizeof(x) for x in (PgGemm, PgTopo, PgSegAttn, PgSegAttnGrad, PgLaunch)]
    if list(sizes) != mine:
        raise RuntimeError(f'phoregen_amd: struct sizes of {path} {list(sizes)} differ from the ctypes mirrors {mine} '
                           '(PgGemm, PgTopo, PgSegAttn, PgSegAttnGrad, PgLaunch)')
    _lib = lib
    return lib


_gpu_checked = False


def lib():
    """The library, for compute calls: additionally requires a visible GPU (checked once, then cached)."""
    global _gpu_checked
    if _gpu_checked:
        return _lib
    l = load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('phoregen_amd: no MI355X / ROCm device visible; the HIP path has no CPU fallback.')
    _gpu_checked = True
    return l


class OrderPoint:
    """A point of one stream that other streams of the same device can wait for (pg_order_point_*: a HIP event without timestamp
    and without the host-visibility fence).  Same two calls as torch.cuda.Event, so the engine can take either."""
    __slots__ = ('h', '_lib')

    def __init__(self):
        self._lib = lib()
        self.h = C.c_void_p()
        check(self._lib.pg_order_point_create(C.byref(self.h)), 'pg_order_point_create')

    def record(self, stream):
        if self._lib.pg_order_point_record(self.h, stream.cuda_stream):
            check(1, 'pg_order_point_record')

    def wait(self, stream):
        if self._lib.pg_order_point_wait(self.h, stream.cuda_stream):
            check(1, 'pg_order_point_wait')

    def __del__(self):
        # (at interpreter shutdown the runtime -- and this module's globals -- may already be gone: the process's events go with it)
        try:
            if self.h and not sys.is_finalizing():
                self._lib.pg_order_point_destroy(self.h)
                self.h = None
        except Exception:
            pass


def launch_record(fn, args, lane):
    """One call of the launch list as a PgLaunch: the arguments as ctypes would pass them (without the trailing stream)."""
    L = PgLaunch()
    L.op, L.lane, L.ev, L.n_arg = PROGRAM_OPS[fn.__name__], lane, -1, len(args)
    assert len(args) == len(fn.argtypes) - 1 <= PG_LAUNCH_MAX_ARGS, fn.__name__
    for i, (a, ty) in enumerate(zip(args, fn.argtypes)):
        if a is None:
            v = 0
        elif ty is C.c_float:
            v = int.from_bytes(struct.pack('<f', a.value if isinstance(a, C.c_float) else float(a)), 'little')
        elif hasattr(a, '_obj'):                    # byref(struct): the struct's address (the engine keeps the struct alive)
            v = C.addressof(a._obj)
        elif isinstance(a, C._SimpleCData):
            v = a.value or 0
        else:
            v = int(a)
        L.a[i] = v & 0xFFFFFFFFFFFFFFFF
    return L


class Program:
    """A launch list inside the library (pg_program_*): one foreign call per run."""
    __slots__ = ('h', '_lib', 'n')

    def __init__(self, records, n_events):
        self._lib = lib()
        arr = (PgLaunch * max(len(records), 1))(*records)
        self.h = C.c_void_p()
        check(self._lib.pg_program_create(arr, len(records), n_events, C.byref(self.h)), 'pg_program_create')
        self.n = len(records)

    def run(self, stream_ptrs):
        if self._lib.pg_program_run(self.h, stream_ptrs):
            check(1, 'pg_program_run')

    def __del__(self):
        try:
            if self.h and not sys.is_finalizing():
                self._lib.pg_program_destroy(self.h)
                self.h = None
        except Exception:
            pass


def form_name(f):
    """A PgSegForm as text: family, row tiles, threads of every launch, composite parts, record width --
    e.g. 'node_fused/t2/768', 'fold+generic/256+unfold', '2x node_two_pass/t2/256/rec16', 'bwd_channel_split/t2/512+t3/256'."""
    one = lambda tiles, threads: (f't{tiles}/' if tiles else '') + str(threads)
    name = FORM_NAMES[f.family]
    if f.family != FORM_NONE:
        name += '/' + one(f.tiles, f.threads)
    if f.threads2:
        name += '+' + one(f.tiles2, f.threads2)
    if f.record_floats:
        name += f'/rec{f.record_floats}'
    if f.compose & PG_FORM_FOLD_UNFOLD:
        name = 'fold+' + name + ('' if f.mode in (SEG_KNN_POS, SEG_BOND_POS) else '+unfold')
    if f.compose & PG_FORM_TWO_LISTS:
        name = '2x ' + name
    return name


def seg_form(topo_ref, s, grad=None):
    """The PgSegForm the library resolves for a PgSegAttn (forward) or a PgSegAttn + PgSegAttnGrad (adjoint); raises on PG_ERR_ARG.
    Host arithmetic: no GPU is touched."""
    f, l = PgSegForm(), load_library()
    if grad is None:
        check(l.pg_seg_attn_form(topo_ref, C.byref(s), C.byref(f)), 'pg_seg_attn_form')
    else:
        check(l.pg_seg_attn_bwd_form(topo_ref, C.byref(s), C.byref(grad), C.byref(f)), 'pg_seg_attn_bwd_form')
    return f


def check(rc, what=''):
    if rc != 0:
        msg = load_library().pg_last_error().decode()
        raise RuntimeError(f'phoregen_hip {what} failed ({rc}): {msg}')


def ptr(t):
    """Device pointer of a tensor (or None)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream
