/*
 * phoregen_hip.h — C ABI of libphoregen_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for PhoreGen's diffusion-denoising hot path.  The reference has no native code
 * (SURVEY.md 2.1): the arithmetic these entry points replace lives in PyTorch op chains and in the
 * un-vendored wheels torch-scatter / torch-sparse / torch-cluster.  Each entry point cites the
 * reference interface it stands in for (file:line under /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed for the duration of the call; the library allocates
 *     nothing and keeps nothing (workspaces are passed in by the caller);
 *   - fp32 row-major tensors, int32 indices;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*), no host synchronisation;
 *   - return value: 0 = ok, otherwise pg_last_error() describes the failure.
 *
 * Context ("ctx") node order is the reference's compose_context order (models/common.py:180-208):
 * per graph, pharmacophore nodes first, then ligand atoms.
 */
#ifndef PHOREGEN_HIP_H
#define PHOREGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* pg_last_error(void);
int pg_abi_version(void);
/* sizeof(PgGemm), sizeof(PgTopo), sizeof(PgSegAttn), sizeof(PgSegAttnGrad), sizeof(PgLaunch) of the library's build -> out[0..n); returns 5.
 * A binding that mirrors the structs (phoregen_amd/hip.py) compares them with its own when it loads the library. */
int pg_abi_struct_sizes(int* out, int n);

/* ---- order points between the HIP streams one denoiser step is spread over (phoregen_amd/engine.py; the reference has no
 * counterpart: it runs on one torch stream).  An event without timestamp whose record is a DEVICE-scope release
 * (hipEventReleaseToDevice) instead of the system-scope fence of a default HIP event: it orders kernels of ONE device against each
 * other, it does not make results visible to the host -- callers synchronise the stream itself for that. */
int pg_order_point_create(void** ev);
int pg_order_point_destroy(void* ev);
int pg_order_point_record(void* ev, void* stream);
int pg_order_point_wait(void* ev, void* stream);          /* `stream` continues after the last record of `ev` */
/* 0 (default): hipEventDisableTiming | hipEventReleaseToDevice, HIP's documented device-scope release at the record.
 * 1 (measurement only, tools/): hipEventDisableTiming | hipEventDisableSystemFence, the round-4 form whose record carries no release
 * of its own.  Applies to order points created afterwards.  Refused (PG_ERR_ARG) unless the process runs with PHOREGEN_DEBUG=1. */
int pg_debug_order_point_fence_free(int on);

/* ---- one denoiser forward as ONE call: a pre-built launch list walked on the host side of the library ---------------------------
 * (reference: the ~3 000 torch ops one `self.forward` of the loop at models/diffusion.py:432-447 issues from Python.)
 * A PgLaunch stands for one entry point of this header (`op`), its arguments `a[0 .. n_arg)` in declaration order WITHOUT the
 * trailing stream -- pointers and integers as 64-bit values, a float as its bit pattern in the low 32 bits -- and the lane it is
 * enqueued on: streams[lane] of pg_program_run.  PG_OP_RECORD / PG_OP_WAIT are the order points between the lanes: `ev` indexes
 * events the program owns (pg_order_point_create flags).  Structs an argument points to (PgGemm, PgSegAttn, PgTopo) are NOT copied:
 * they, and every device buffer, must outlive the program. */
enum {
  PG_OP_RECORD = 0, PG_OP_WAIT = 1, PG_OP_GEMM = 2, PG_OP_SEG_ATTN = 3, PG_OP_EMBED_CTX = 4, PG_OP_EMBED_BOND = 5, PG_OP_KNN_CTX = 6,
  PG_OP_LIG_NORMALS = 7, PG_OP_EDGE_GATE = 8, PG_OP_KNN_GROUP_BY_KIND = 9, PG_OP_BOND_SMEAR = 10, PG_OP_ATTN_FOLD_QUERY = 11,
  PG_OP_ATTN_UNFOLD_VALUE = 12, PG_OP_APPLY_DX = 13, PG_OP_LAYER_GEOM = 14, PG_OP_ROWS_LINEAR = 15, PG_OP_ATOM_COUNT = 16,
  PG_OP_EMBED_BOND_E16 = 17
};
#define PG_PROGRAM_LANES 4
#define PG_LAUNCH_MAX_ARGS 12
typedef struct {
  int32_t op;                          /* PG_OP_* */
  int32_t lane;                        /* 0 .. PG_PROGRAM_LANES-1 */
  int32_t ev;                          /* PG_OP_RECORD / PG_OP_WAIT: order point index */
  int32_t n_arg;
  uint64_t a[PG_LAUNCH_MAX_ARGS];
} PgLaunch;
int pg_program_create(const PgLaunch* list, int n, int n_events, void** prog);   /* validates and copies the list, creates the events */
int pg_program_run(void* prog, void* const* streams /*[PG_PROGRAM_LANES] hipStream_t*/);
/* (a failing entry leaves the lanes half-enqueued: the call then drains the device, marks the program POISONED and returns the entry's
 *  error; every later run of a poisoned program is refused -- the owner destroys it and rebuilds its state) */
int pg_program_length(void* prog);
int pg_program_destroy(void* prog);

/* ---- measurement aid: `workgroups` x 4 waves issue `iters` x 16 v_mfma_f32_16x16x4_f32 each (8 independent chains) and nothing else;
 * *flops (host, optional) = the FLOPs of the launch.  bench.py times it with HIP events: the fp32 matrix rate this GPU sustains,
 * quoted beside the nominal peak.  1024 workgroups = 4 waves per SIMD of 256 CUs. */
int pg_micro_mfma_f32(int workgroups, int iters, float* sink, double* flops, void* stream);

/* ---- MFMA lane-map self test (device writes 0 on success) -------------------------------- */
int pg_selftest_mfma(int* d_result, void* stream);
/* ---- raw words of the device generator (Philox4x32-10, Salmon et al. SC'11) for known-answer tests:
 * ctr_key [n][6] = counter c0..c3, key k0 k1  ->  out [n][4].  The transition kernels call it with
 * key = seed (lo, hi), counter = (element index lo, hi, step, stream_id). */
int pg_selftest_philox(const uint32_t* ctr_key, int n, uint32_t* out, void* stream);
/* test hook (returns the old setting): bit 0 routes the node-target modes of pg_seg_attn through the generic one-pass kernel,
 * bit 1 no longer has an effect (it selected a triplet kernel that has since been removed),
 * bit 2 runs the staged kernel with 8 instead of 12 waves per workgroup (tuning) */
int pg_debug_force_generic_seg(int mask);

/* ---- dense linear layers -------------------------------------------------------------------
 * Y[R, n] = out_scale * act( sum_k Xcat[R,k] * W[n,k] + bias[n] + add1[i1(r), n] + add2[i2(r), n] ),  R = rows ? rows[r] : r
 * Xcat = [X | X2] along k; if ln_gamma != NULL, X rows first go through LayerNorm(K1, eps 1e-5)+ReLU.
 * Replaces nn.Linear / MLP second halves (models/common.py:99-119), the per-node / per-edge halves
 * of the first MLP layer that the reference computes on concatenated gathers
 * (models/uni_denoiser.py:43-59,141-155,190-201), lin_node (:288) and the heads
 * (models/diffusion.py:55-59,71-75,223,241). */
typedef struct {
  const float* X;   int ldx;  int K1;
  const float* X2;  int ldx2; int K2;
  const float* W;   int ldw;
  const float* bias;
  const float* ln_gamma; const float* ln_beta;
  const float* add1; int ld_add1; const int* idx1;
  const float* add2; int ld_add2; const int* idx2;
  float out_scale;
  int   act;                 /* 0 none, 1 shifted softplus (models/common.py:58-64), 2 ReLU */
  float* Y; int ldy; int M; int N;
  const int* rows;           /* optional [M]: logical row r reads X/X2 row rows[r] and writes Y row rows[r] (row subset) */
  int add_rows;              /* rows of add1 / add2 (upper bound of idx1 / idx2 values + 1); 0 = unknown.  Lets pg_gemm pick the
                              * streaming kernel, which addresses the gathered rows with 32-bit byte offsets */
  int row_extent;            /* with tile_rows: rows of the X / Y buffers (every window lies inside [0, row_extent)) */
  const int* tile_rows;      /* optional [M / 64], device-accessible: row windows.  The product runs over M / 64 windows of 64 consecutive
                              * rows; window t covers rows tile_rows[t] .. tile_rows[t] + 63 of X and of Y (row r of Y from row r of X, so
                              * overlapping windows write the same bits) and M counts the rows computed.  Every first row must lie in
                              * [0, row_extent - 64]: checked when the list is host-visible (pinned or managed memory), the caller's duty
                              * for a device-only list.  Streaming kernel only: K1 = 128, K2 = 0, no added operand, no `rows`, act = 0, N a
                              * multiple of 128 (plain or LayerNorm-on-load with N = 128); anything else is an error, not a slower path */
} PgGemm;
int pg_gemm(const PgGemm* p, void* stream);
/* test hook (returns the old setting): 0 keeps every product on the tiled kernel (csrc/gemm.hip) instead of the streaming one
 * (csrc/gemm_stream.hip), so that the tests can hold the two against each other (a product with row windows, `tile_rows`, has no tiled
 * form and stays on the streaming kernel) */
int pg_debug_gemm_streaming(int on);
/* which kernel pg_gemm launches for *p under the current setting of the hook: 1 the streaming kernel, 0 the tiled one (host arithmetic) */
int pg_gemm_is_streaming(const PgGemm* p);

/* ---- graph topology of one batch ------------------------------------------------------------
 * Built once per batch by the host mirror (phoregen_amd/plan.py); constant over the 1000 steps. */
typedef struct {
  int n_graphs, n_ctx, n_lig, n_phore, n_bond;
  int max_nlig;             /* largest ligand of the batch (selects the triplet kernel variant)           */
  int max_gctx;             /* most context nodes (ligand + pharmacophore) of any graph; pg_knn_ctx holds <= 512 */
  const int* g_ctx_off;     /* [B+1] first ctx node of graph g                                   */
  const int* g_nph;         /* [B]   pharmacophore nodes of graph g (ctx rows g_ctx_off[g]..+nph) */
  const int* g_nlig;        /* [B]   ligand atoms of graph g (follow the phore nodes)             */
  const int* g_eid_off;     /* [B+1] offset of graph g's n_lig x n_lig edge-id table in `eid`     */
  const int* eid;           /* eid[off_g + a_src*n + a_dst] = bond edge id, -1 on the diagonal    */
  const int* ctx_graph;     /* [n_ctx] graph of a ctx node                                        */
  const uint8_t* ctx_is_lig;/* [n_ctx]                                                            */
  const int* lig2ctx;       /* [n_lig] ctx index of ligand atom a (= l_index_in_ctx, common.py:166-177) */
  const int* bond_src;      /* [n_bond] ctx index of edge source (edge_index[0], diffusion.py:201) */
  const int* bond_dst;      /* [n_bond] ctx index of edge target                                  */
  const int* bond_desc;     /* [n_bond][4] {ctx j, local_i | local_j << 16, n_lig of the graph, eid offset of the graph} */
  const int* g_bond_off;    /* [B+1] first bond row of graph g                                    */
  const int* edge_ref;      /* [n_bond] or NULL: bond rows inside the library are in the host mirror's INTERNAL order (per graph
                               target-major: the edges k -> i of one target i are contiguous, k ascending; phoregen_amd/plan.py);
                               edge_ref[e] = row of internal edge e in the caller's edge arrays (h_edge_pert, h_edge_prev).
                               NULL: the caller's order already is the internal one */
} PgTopo;

/* ---- embeddings (models/diffusion.py:180-183,205; models/common.py:34-55) -------------------- */
int pg_embed_ctx(const PgTopo* t, const float* h_node_pert /*[n_lig,12]*/, const float* pos_pert /*[n_lig,3]*/,
                 const int64_t* time_step /*[B]*/, const float* W_node /*[118,12]*/,
                 const float* t_offset /*[10]*/, const float* t_coeff /*[10]*/,
                 const float* h_phore_emb /*[n_phore,128]*/, const float* pos_phore /*[n_phore,3]*/,
                 const int* phore2ctx /*[n_phore]*/, float* h_ctx /*[n_ctx,128]*/, float* x_ctx /*[n_ctx,3]*/,
                 void* stream);      /* h_ctx == NULL / x_ctx == NULL: that half is skipped (the features of the NEXT reverse step are embedded
                                        as soon as its types are drawn, the coordinates when its positions are: phoregen_amd/engine.py) */
int pg_embed_bond(const PgTopo* t, const float* h_edge_pert /*[n_bond,6], caller's order (t->edge_ref)*/, const int* bond_graph,
                  const int64_t* time_step, const float* W_edge /*[118,6]*/, const float* t_offset,
                  const float* t_coeff, float* h_bond /*[n_bond,128], 16-byte aligned (PG_ERR_ARG otherwise)*/, void* stream);
/* pg_embed_bond with a second, optional output: e16[e] = [ h_edge_pert of internal edge e (6) | the 10 time-smearing values of its graph ],
 * the 16 numbers a row of h_bond is linear in (the very floats of h_bond[e, 118:128]).  Layer 0's bond-row products run over e16 with
 * composed weights (phoregen_amd/packing.py: l0_compose).  e16 == NULL: pg_embed_bond.  h_bond and e16 must be 16-byte aligned */
int pg_embed_bond_e16(const PgTopo* t, const float* h_edge_pert, const int* bond_graph, const int64_t* time_step, const float* W_edge,
                      const float* t_offset, const float* t_coeff, float* h_bond /*[n_bond,128]*/, float* e16 /*[n_bond,16] or NULL*/,
                      void* stream);

/* ---- neighbour search (torch_cluster.knn_graph via uni_denoiser.py:355 and common.py:301) ----
 * pg_knn_ctx: k nearest other ctx nodes of the same graph -> nbr[n_ctx,k] (ascending distance, index
 *   breaks ties), deg[n_ctx] = min(k, nodes_in_graph-1).
 * pg_lig_normals: nrm[ctx] = mean of the 3 nearest ligand atoms' positions - x  for ligand atoms
 *   (common.py:300-304), phore_norm rows for pharmacophore nodes (common.py:312-314). */
int pg_knn_ctx(const PgTopo* t, const float* x_ctx, int k, int* nbr, int* deg, void* stream);
int pg_lig_normals(const PgTopo* t, const float* x_ctx, const float* phore_norm, const int* phore2ctx,
                   float* nrm, void* stream);

/* nn3[n_lig,3]: ctx ids of the neighbours pg_lig_normals averages (-1 = fewer than 3 other atoms); training path */
int pg_lig_nn3(const PgTopo* t, const float* x_ctx, int* nn3, void* stream);

/* global edge gate e_w = sigmoid(MLP(smear(dist)))  (uni_denoiser.py:410-415); weights in kernel layout
 * (phoregen_amd/packing.py pack_gate): W0 = lane-fixed centred/sign-normalised first layer [5][8][64], b0 = its bias
 * [128], gamma unused, beta = beta/|gamma| [128], W3 = last-layer row times |gamma| [128] */
int pg_edge_gate(const PgTopo* t, const float* x_ctx, const int* nbr, const int* deg, int k,
                 const float* W0, const float* b0, const float* gamma, const float* beta,
                 const float* W3, float b3, float* ew /*[n_ctx,k]*/, void* stream);

/* optional, after pg_edge_gate: stable partition of every node's neighbour slots (and their gate values) by the kind of the source
 * node, ligand atoms first.  The attention kernels sum over a node's rows, so the order is free; with it at most one 16-row tile
 * per node mixes the two kinds and the uniform tiles skip the other kind's 20 distance columns (csrc/node_attn.hip). */
int pg_knn_group_by_kind(const PgTopo* t, int k, int* nbr /*[n_ctx,k] in place*/, const int* deg, float* ew /*[n_ctx,k] in place*/,
                         void* stream);

/* per-bond Gaussian smearing of the bond length: G[e, 0:20] (uni_denoiser.py:128,137) */
int pg_bond_smear(const PgTopo* t, const float* x_ctx, float* G /*[n_bond,20]*/, void* stream);

/* ---- segment attention (the hot path) --------------------------------------------------------
 * One call = one attention sub-layer of AttentionLayerO2TwoUpdateNodeGeneral (uni_denoiser.py:260-298)
 * with the MLP first layers factored (SURVEY.md 7 "hard parts"):
 *   hidden_m[row] = Csrc_m[src_row(row)] + Cdst_m[segment] + Wf_m * feat(row)          m in {k, v}
 *   z_m = ReLU(LayerNorm(hidden_m));  logits[row,h] = z_k . U[segment][:,h]
 *   alpha = softmax over the rows of a segment;  S[segment][:,h] = sum_row alpha*gate * z_v
 * U / S are the per-segment query-folded key weights and value pre-images.
 * Modes: */
enum {
  PG_SEG_KNN_NODE = 0,   /* NodeUpdateLayer on knn edges      (uni_denoiser.py:40-72 via :281)  */
  PG_SEG_KNN_POS  = 1,   /* PosUpdateLayer  on knn edges      (uni_denoiser.py:187-209 via :291) */
  PG_SEG_BOND_NODE = 2,  /* NodeUpdateLayer on bond edges     (:284)                             */
  PG_SEG_BOND_POS  = 3,  /* PosUpdateLayer  on bond edges     (:294)                             */
  PG_SEG_TRIPLET   = 4,  /* BondUpdateLayer                   (uni_denoiser.py:101-165 via :285) */
  PG_SEG_PHORE     = 5   /* phore encoder NodeUpdateLayer     (diffusion.py:186-191)             */
};

typedef struct {
  int mode;
  int n_seg;
  const int* seg_ids;        /* [n_seg] ctx node ids (node modes); triplet: bond edge ids in visiting order, NULL = 0..n_seg-1 */
  const int* seg_chunks;     /* triplet: [257] cost-balanced segment ranges, one per workgroup; NULL = equal split */
  /* geometry */
  const float* x;            /* [n_ctx,3] positions the features are computed from               */
  const float* nrm;          /* [n_ctx,3] direction vectors (knn modes)                          */
  const int* nbr; const int* deg; const float* ew; int knn_k;   /* knn modes                      */
  /* factored first layer */
  const float* Csrc_k; const float* Csrc_v; int ld_csrc;
  const float* Cdst_k; const float* Cdst_v; int ld_cdst;
  const float* Wf_k; const float* Wf_v;  /* lane-fixed [F/4][8][64] feature weights; node modes: 16-byte aligned (as are Wf_k2,
                                            Wf_v2 and W2xv_l: the tables go to LDS in 16-byte pieces; PG_ERR_ARG otherwise) */
  const float* Wg2_k; const float* Wg2_v;/* triplet: [20][128] weights of smear(d_ji)             */
  const float* G;                        /* triplet: [n_bond,20] from pg_bond_smear               */
  const float* ln_gk; const float* ln_bk; const float* ln_gv; const float* ln_bv;
  /* attention */
  const float* U;            /* node modes: [n_ctx][32][64] lane-fixed U (pg_attn_fold_query)      */
  const float* q;            /* triplet: [n_bond,128] queries, pre-scaled by 1/sqrt(head_dim)      */
  const float* W2k_l;        /* triplet: lane-fixed second-layer key weights [64][64][4]           */
  const float* W2v_l; const float* b2v;      /* triplet: lane-fixed value weights + bias          */
  /* Fused form of the four node modes (the sampler): q [n_ctx,128] and W2k_l given -> the query is folded in-kernel and U is not
   * read; the node-update modes (KNN_NODE, BOND_NODE) given W2v_l, b2v and out [n_ctx,128] (rows 128 floats apart) also apply
   * the value second layer and write out[seg,:] = W2v . S + b2v * sum(alpha * gate) instead of S / swn, i.e. what
   * pg_attn_fold_query -> pg_seg_attn -> pg_attn_unfold_value compute as three launches.  U (and S, swn) must still point at
   * scratch of the plain form's size: shapes the two-pass kernels do not hold (knn_k > 32, ligands above 80 atoms) run the
   * three launches internally. */
  const float* W2xv_l; const float* b2xv;    /* pos modes: lane-fixed [32][64] + [16]             */
  /* outputs */
  float* S; float* swn;      /* node modes: [n_ctx][32][64], [n_ctx][16]                          */
  const float* resid; float* out;            /* triplet: out[e,:] = resid[e,:] + update           */
  float* dx;                 /* pos modes: [n_ctx,3]                                              */
  int accumulate_dx;         /* pos modes: dx += instead of =                                     */
  float* alpha; int alpha_rows; /* optional (training): triplet S-form and the node-update modes of csrc/node_attn.hip write the
                                   softmax weights (x gate) [segments][alpha_rows][16]; its position modes write the logits and the
                                   value scalars of every row [segments][alpha_rows][32] -- what PgSegAttnGrad.alpha takes         */
  /* PG_SEG_PHORE, optional: the scalar edge feature given explicitly instead of computed as |x_dst - x_src| (the standalone
   * NodeUpdateLayer.forward(h, edge_feat, edge_index) of models/uni_denoiser.py:40-72 receives it from its caller):
   * efeat[efeat_off[g] + src_local * p_g + dst_local] for graph g with p_g nodes = the order of
   * fully_connect_two_graphs (models/common.py:329-356).  NULL: distances from `x`. */
  const float* efeat; const int* efeat_off;
  /* PG_SEG_TRIPLET, optional: source-atom groups for the LDS-staged kernel (csrc/triplet2.hip).  tri_iters [n_tri_iters][4] =
   * {ctx index of the ligand's first atom, n | j0 << 8 | A << 16, first internal bond row of the graph, s0 | s1 << 16}: the A
   * consecutive source atoms j0.. of an n-atom ligand, A*(n-1) <= 80, longest first; the entry covers the segments [s0, s1) of the
   * group's A*(n-1) (0: all of them); tri_counter: TWO ints of scratch (queue head, exit count), zero before the first launch --
   * every launch leaves them zero again.
   * Requires the target-major bond order of the host mirror, Csrc_k/Csrc_v = the two halves of one [n_bond,256] tensor and
   * Cdst_k/Cdst_v [n_bond] rows = smear(d_ji) . Wg2 of the segment's own edge (as in the adjoint's contract). */
  const int* tri_iters; int n_tri_iters; int* tri_counter;
  /* Fused knn modes, optional: a SECOND target list served by the same launch (the pharmacophore targets beside the ligand targets
   * of one sub-layer; they differ in the feature weights only): seg_ids2 [n_seg2], Wf_k2 / Wf_v2.  The persistent workgroups are
   * split between the two lists in proportion to their sizes, so that the two lists finish together instead of each rounding
   * its own number of node rounds up (one launch instead of two).  n_seg2 = 0: one list. */
  const int* seg_ids2; int n_seg2; const float* Wf_k2; const float* Wf_v2;
  /* PG_SEG_TRIPLET with tri_iters, optional: persistent workgroups of the staged kernel (0 = one per CU, 256).  A small batch
   * leaves some CUs to the launches that run beside the triplet kernel on other streams: 16 graphs of the headline shape 3.76 ->
   * 3.57 ms per step with 200 workgroups (the results do not depend on it: the queue hands out the same segments). */
  int tri_grid;
  /* Fused position modes (KNN_POS, BOND_POS), optional: 1 = the row tiles of a node over several waves of a workgroup (a small
   * batch's launch of a few hundred nodes is bound by the dependent chain inside the one wave that owns a node); the sequential
   * chains are run in the one-wave kernel's order, so the result is bit-identical.  Ignored for shapes it does not hold (ligands
   * above 64 atoms, k > 32, training outputs): those take the one-wave kernel. */
  int pos_tiled;
  /* PG_SEG_TRIPLET with tri_iters, optional: the largest ligand (atoms) among the queue's entries when that is smaller than
   * PgTopo.max_nlig.  The staged kernel is instantiated for the row tiles of the largest ligand it may meet, and the 4-tile
   * instance costs EVERY segment ~4 % (44 instead of 31 spilled registers): a batch with a few 51+-atom ligands (a segment visits n - 2 rows) runs them as a
   * second launch with its own queue and the rest on the 3-tile instance.  0 = PgTopo.max_nlig. */
  int tri_max_nlig;
} PgSegAttn;
int pg_seg_attn(const PgTopo* t, const PgSegAttn* p, void* stream);

/* ---- which kernel serves a pg_seg_attn / pg_seg_attn_bwd call --------------------------------
 * The limits of the kernel forms, by name (phoregen_amd/hip.py mirrors them; the kernel files take them from here).  A row tile
 * is 16 rows of a segment; "tiles" below is ceil(rows / 16) of the largest segment a launch may meet. */
#define PG_SEG_ROW_TILE 16
#define PG_SEG_KNN_MAX_K 32             /* knn modes: the node kernels (csrc/node_attn.hip) hold 2 row tiles, knn_k up to 32          */
#define PG_SEG_NODE_MIN_TILES 3         /* bond modes: the node kernels are built for 3, 4 and 5 row tiles of PgTopo.max_nlig ...     */
#define PG_SEG_NODE_MAX_TILES 5         /* ... ligands of up to 80 atoms                                                              */
#define PG_SEG_POS_TILED_MIN_TILES 2    /* PgSegAttn.pos_tiled: built for 2, 3 and 4 row tiles ...                                    */
#define PG_SEG_POS_TILED_MAX_TILES 4    /* ... ligands of up to 64 atoms                                                              */
#define PG_SEG_TRI_STAGED_ROWS 80       /* staged triplet kernel (csrc/triplet2.hip): rows of P a workgroup stages, max_nlig - 1 <= 80 */
#define PG_SEG_TRI_STAGED_ATOMS 96      /* ... and ligand atoms whose coordinates it stages                                           */
#define PG_SEG_TRI_STAGED_LD 256        /* ... ld_csrc of its one [n_bond, 256] = [P_k | P_v] tensor, Csrc_v == Csrc_k + 128           */
#define PG_SEG_TRI_MIN_TILES 3          /* ... built for 3, 4 and 5 row tiles of the n - 2 rows a segment visits                      */
#define PG_SEG_TRI_MAX_TILES 5
#define PG_SEG_TRI_WAVES 12             /* ... on 12 waves per workgroup ...                                                          */
#define PG_SEG_TRI_WAVES_DEBUG 8        /* ... or 8 (sampling form, pg_debug_force_generic_seg bit 2)                                 */
#define PG_SEG_BWD_TRI_MAX_ATOMS 64     /* triplet adjoint: 4 waves per workgroup, the two-pass and the channel-split form up to 64
                                           atoms of PgTopo.max_nlig; above, the one-wave form on 2 waves                              */
#define PG_SEG_BWD_TRI_FORM2_ATOMS 32   /* PgSegAttnGrad.tri_form 2: ligands up to 32 atoms on the 8-wave launch                      */
#define PG_SEG_BWD_LDS_BYTES 163840     /* the adjoint's LDS budget; for the triplet's one-wave form that is                          */
#define PG_SEG_BWD_TRI_BASE_FLOATS 7680 /* ... weight tables and accumulators of a workgroup ...                                      */
#define PG_SEG_BWD_TRI_WAVE_FLOATS 3072 /* ... + per wave ...                                                                         */
#define PG_SEG_BWD_TRI_ROW_FLOATS 259   /* ... + per atom of max_nlig rounded up to a row tile: refused (PG_ERR_ARG) when it is more  */
#define PG_SEG_PHORE_RECORD_ROWS 256    /* training path: pharmacophore graphs up to this size ask the forward for its per-row record */

/* kernel families (PgSegForm.family) and the file that holds the kernel */
enum {
  PG_FORM_NONE = 0,               /* nothing is launched: no segments                                                               */
  PG_FORM_GENERIC = 1,            /* one-pass, one wave per segment, any shape             seg_attn.hip    seg_attn_kernel<mode>     */
  PG_FORM_NODE_TWO_PASS = 2,      /* node modes, U given                                   node_attn.hip   node_attn_kernel<.., false> */
  PG_FORM_NODE_FUSED = 3,         /* node modes, query fold (and value unfold) in-kernel   node_attn.hip   node_attn_kernel<.., true> */
  PG_FORM_POS_TILED = 4,          /* fused position modes, a node's row tiles over waves   node_attn.hip   node_attn_pos_tiled_kernel */
  PG_FORM_TRI_STAGED = 5,         /* triplet, sampling: out = resid + update               triplet2.hip    triplet2_kernel<.., false> */
  PG_FORM_TRI_STAGED_TRAIN = 6,   /* triplet, training: S, swn (and the record)            triplet2.hip    triplet2_kernel<.., true> */
  PG_FORM_BWD_ONE_WAVE = 7,       /* adjoint, one wave per row tile, both MLP paths        seg_attn_bwd.hip seg_attn_bwd_kernel<.., 0> */
  PG_FORM_BWD_TWO_PASS = 8,       /* adjoint as a value pass, then a key pass              seg_attn_bwd.hip seg_attn_bwd_kernel<.., 1 / 2> */
  PG_FORM_BWD_CHANNEL_SPLIT = 9   /* triplet adjoint, a tile's channels over the waves     triplet_bwd2.hip triplet_bwd2_kernel       */
};
/* composite cases (PgSegForm.compose, a bit set) */
#define PG_FORM_TWO_LISTS 1      /* forward: the two target lists are served one after the other, each in the form described        */
#define PG_FORM_FOLD_UNFOLD 2    /* forward: a fused request served as pg_attn_fold_query + the form described (+ pg_attn_unfold_value
                                    in the node-update modes)                                                                       */
#define PG_FORM_SECOND_LAUNCH 4  /* adjoint, tri_form 2: the 8-wave launch (tiles, threads), then the 4-wave launch (tiles2, threads2)
                                    for the ligands of more than PG_SEG_BWD_TRI_FORM2_ATOMS atoms                                   */
/* What a call runs.  Two calls with equal PgSegForm run the same code: (mode, family, tiles, threads, record_floats) name the template
 * instantiation, compose / tiles2 / threads2 the launches around or after it. */
typedef struct {
  int mode;            /* PG_SEG_*                                                                                                  */
  int family;          /* PG_FORM_*                                                                                                 */
  int tiles;           /* row tiles the kernel is instantiated for; 0: the family is not instantiated per tile count                */
  int threads;         /* threads per workgroup (64 per wave); PG_FORM_BWD_TWO_PASS: of the value pass                              */
  int compose;         /* PG_FORM_TWO_LISTS | PG_FORM_FOLD_UNFOLD | PG_FORM_SECOND_LAUNCH                                           */
  int tiles2;          /* second launch of the same family (PG_FORM_SECOND_LAUNCH; the key pass of PG_FORM_BWD_TWO_PASS) ...        */
  int threads2;        /* ... 0: there is none                                                                                      */
  int record_floats;   /* forward: floats per row the launch leaves at PgSegAttn.alpha (16: softmax weights, 32: logits | value
                          scalars, 0: no record); adjoint: floats per row of the record it reads from PgSegAttnGrad.alpha           */
  int rowbuf_waves;    /* adjoint: waves per workgroup PgSegAttnGrad.rowbuf must be sized for; 0: the form has no row buffer        */
} PgSegForm;
/* Host arithmetic only (no GPU needed, nothing is dereferenced): the form pg_seg_attn / pg_seg_attn_bwd would run for these
 * arguments, or PG_ERR_ARG with the message of the entry point for everything it refuses by its argument and LDS checks.
 * Honours pg_debug_force_generic_seg. */
int pg_seg_attn_form(const PgTopo* t, const PgSegAttn* p, PgSegForm* out);

/* U[s][c][h] = sum_d q[s,8h+d] * W2k[8h+d,c]  in lane-fixed layout (key second layer folded into the query) */
int pg_attn_fold_query(const float* q /*[n,128] pre-scaled*/, int ldq, const float* W2k_l, int n,
                       const int* ids, float* U, void* stream);
/* out[s, 8h+d] = sum_c W2v[8h+d,c] * S[s][c][h] + b2v[8h+d] * swn[s][h]   (swn / b2v NULL: no bias term) */
int pg_attn_unfold_value(const float* S, const float* swn, const float* W2v_l, const float* b2v, int n,
                         const int* ids, float* out, int ldo, void* stream);

/* x_new[i] = x[i] + (dx1[i] + dx2[i]) * is_lig[i]   (uni_denoiser.py:295-296) */
int pg_apply_dx(const PgTopo* t, const float* x, const float* dx1, const float* dx2, float* x_new, void* stream);

/* Everything of a layer that depends on the coordinates only, as ONE launch (the arithmetic of pg_apply_dx, pg_bond_smear and
 * pg_lig_normals, bit for bit): x_new = x + (dx1 + dx2) * is_lig  (uni_denoiser.py:295-296), then FROM x_new the bond-length
 * smearing G[n_bond,20] (uni_denoiser.py:128,137) and the direction vectors nrm[n_ctx,3] (common.py:300-314) the next layer reads.
 * dx1 == dx2 == NULL: no update (x_new unused; G / nrm from x).  G == NULL / nrm == NULL: that product is skipped.
 * nrm_phore_ctx [n_ctx,3]: the pharmacophore normals in ctx row order (rows of ligand atoms unused). */
int pg_layer_geom(const PgTopo* t, const float* x, const float* dx1, const float* dx2, const float* nrm_phore_ctx,
                  float* x_new, float* nrm, float* G, void* stream);

/* small per-row linear: Y[r, 0:n_out] = W[n_out,K] . X[rows ? rows[r] : r, 0:K] + b   (n_out <= 16, K <= 256) */
int pg_rows_linear(const float* X, int ldx, int K, const float* W, const float* b, int n_out, int M,
                   const int* rows, float* Y, int ldy, void* stream);

/* atom-count heads: per graph mean of sigmoid(logit) over all / non-EX phore nodes, u = l + relu(c - l)
 * (diffusion.py:148-163); s_all / s_l are the pre-sigmoid outputs of atom_mlp / atom_mlp_1 */
int pg_atom_count(const float* s_all /*[n_phore]*/, const float* s_l /*[n_phore]*/, const uint8_t* is_ex,
                  const int* phore_graph, int n_phore, int n_graphs, float* count_l, float* count_u, void* stream);

/* ---- reverse-diffusion step (models/transition.py:44-63,285-315, models/common.py:425-431) ----
 * categorical: log_softmax(logits) -> q_v_posterior(v0_prob=True) -> Gumbel-argmax -> one-hot.
 * `uniform` / `eps` != NULL replay given draws (parity mode); NULL -> counter-based Philox4x32-10 with key = seed and
 * counter = (element, step, stream_id).  element = flat index of the batch when graph_row0 == NULL; otherwise the
 * graph-keyed form (graph_key[g] << 32 | index of the element inside graph g), with graph_row0[g] = first row of graph g
 * and graph_key[g] = a caller-chosen id (NULL: g): a graph then draws the same noise in whatever batch or shard it is
 * sampled (per-graph sharding over GPUs reproduces the unsharded run). */
int pg_posterior_categorical(const float* logits, const float* log_vt_in, const int* row_graph,
                             const int64_t* time_step, const float* q_mats, const float* q_onestep_T,
                             int n_rows, int K, const float* uniform, uint64_t seed, uint32_t stream_id,
                             uint32_t step, const int* graph_row0, const int* graph_key, float* log_vt_out,
                             float* onehot_out, float* traj_out, void* stream);
int pg_posterior_position(const float* x_t, const float* x0, const int* row_graph, const int64_t* time_step,
                          const float* coef_x0, const float* coef_xt, const float* std_, const float* energy_grad,
                          const float* eps, uint64_t seed, uint32_t stream_id, uint32_t step, int n_rows,
                          const int* graph_row0, const int* graph_key, const float* center /*[B,3] per graph, added to traj_out only; or NULL*/,
                          float* x_prev, float* traj_out, void* stream);

/* The same step for a sampler loop that keeps the coordinates in the denoiser's ctx-ordered buffers (phoregen_amd/models/diffusion.py,
 * pipelined loop): x0 is read as x0_ctx[lig2ctx[row]] (the denoiser's final coordinate buffer: no gather launch in front), the new
 * position is also written to x_ctx_next[lig2ctx[row]] (the coordinates layer 0 of the NEXT step reads: no embedding launch behind;
 * may be the buffer x0_ctx points to) and x0 itself to x0_out [n_rows,3] (optional).  Same arithmetic, same noise. */
int pg_posterior_position_ctx(const float* x_t, const float* x0_ctx, const int* lig2ctx, const int* row_graph,
                              const int64_t* time_step, const float* coef_x0, const float* coef_xt, const float* std_,
                              const float* energy_grad, const float* eps, uint64_t seed, uint32_t stream_id, uint32_t step,
                              int n_rows, const int* graph_row0, const int* graph_key, const float* center, float* x_prev,
                              float* traj_out, float* x_ctx_next, float* x0_out, void* stream);

/* Fragment-conditioned sampling (beyond the reference): the three posterior entry points above with the fixed rows of a fragment
 * replaced in the same launch.  frag_cls [n_rows]: the fixed class of a row, -1 = free (free rows: exactly the plain entry point's
 * results).  A fixed row is redrawn at level lvl = time_step - 1 from the forward process: types by Gumbel-argmax over
 * log q_mats[lvl][v0,:] (floored at -32; log_vt_out = that log-distribution), coordinates sqrt_ab[lvl] * x0f + sqrt_1mab[lvl] * eps;
 * at time_step 0 the fragment itself (class v0, log-state 0 / -32; coordinates x0f).  Noise: the same Philox and the same counters
 * as the posterior, with stream id frag_stream_id and counter step lvl (the replacement uses Philox even when `uniform` / `eps`
 * are given).  x0f [n_rows,3]: fragment coordinates minus the graph's centre; sqrt_ab / sqrt_1mab [T]. */
int pg_posterior_categorical_frag(const float* logits, const float* log_vt_in, const int* row_graph,
                                  const int64_t* time_step, const float* q_mats, const float* q_onestep_T,
                                  int n_rows, int K, const float* uniform, uint64_t seed, uint32_t stream_id,
                                  uint32_t step, const int* graph_row0, const int* graph_key, float* log_vt_out,
                                  float* onehot_out, float* traj_out, const int* frag_cls, uint32_t frag_stream_id, void* stream);
int pg_posterior_position_frag(const float* x_t, const float* x0, const int* row_graph, const int64_t* time_step,
                               const float* coef_x0, const float* coef_xt, const float* std_, const float* energy_grad,
                               const float* eps, uint64_t seed, uint32_t stream_id, uint32_t step, int n_rows,
                               const int* graph_row0, const int* graph_key, const float* center, float* x_prev, float* traj_out,
                               const int* frag_cls, const float* x0f, const float* sqrt_ab, const float* sqrt_1mab,
                               uint32_t frag_stream_id, void* stream);
int pg_posterior_position_ctx_frag(const float* x_t, const float* x0_ctx, const int* lig2ctx, const int* row_graph,
                                   const int64_t* time_step, const float* coef_x0, const float* coef_xt, const float* std_,
                                   const float* energy_grad, const float* eps, uint64_t seed, uint32_t stream_id, uint32_t step,
                                   int n_rows, const int* graph_row0, const int* graph_key, const float* center, float* x_prev,
                                   float* traj_out, float* x_ctx_next, float* x0_out, const int* frag_cls, const float* x0f,
                                   const float* sqrt_ab, const float* sqrt_1mab, uint32_t frag_stream_id, void* stream);
/* The replacement alone at one level (-1 = the fragment itself) for every fixed node row (one-hot type, log-state, coordinates) and
 * fixed bond row (one-hot type, log-state), with the counters of the posteriors above (graph_row0 = g_lig_off / g_bond_off, may be
 * NULL: flat counters).  Free rows and NULL outputs are not written.  The sampler's initial state (level T - 1). */
int pg_fragment_noise(int level, uint64_t seed, int n_lig, int n_bond, const int* node_cls, const int* edge_cls,
                      const float* x0f, const int* lig_graph, const int* bond_graph, const int* g_lig_off,
                      const int* g_bond_off, const int* graph_key, const float* q_node, const float* q_edge,
                      const float* sqrt_ab, const float* sqrt_1mab, uint32_t node_stream_id, uint32_t edge_stream_id,
                      uint32_t pos_stream_id, float* h_node, float* log_node, float* h_edge, float* log_edge,
                      float* x_out, void* stream);

/* closed-form guidance gradient (models/diffusion.py:476-502, utils/sample_utils.py:135-165).  phore_center [B,3]: per
 * graph the mean position of its non-EX pharmacophore nodes.  Both energies are means over the graphs of the batch;
 * mean_over_graphs = that divisor (<= 0: this batch's n_graphs; a shard of a larger logical batch passes the full count). */
int pg_guidance_grad(const PgTopo* t, const float* x_lig /*[n_lig,3]*/, const float* h_edge_prev /*[n_bond,6]*/,
                     const int* lig_graph, const int* g_lig_off, int use_atom_prox, float min_d, float max_d,
                     int use_center_prox, const float* phore_center /*[B,3]*/, int mean_over_graphs, float* cnt_ws /*[B]*/,
                     float* mean_ws /*[B,3]*/, float* grad /*[n_lig,3]*/, void* stream);

/* ---- training path: backward kernels (PhoreDiff.compute_loss, models/diffusion.py:249-352) -------------------
 * The forward of a training step runs the same kernels as sampling; these entry points are their adjoints.
 * Gradient buffers marked (+=) are accumulated with atomics into caller-zeroed memory, (=) are overwritten. */

/* gW[n,k] (+=) sum_r dY[r,n] * X[r,k];  gb[n] (+=) sum_r dY[r,n] (gb may be NULL).  Adjoint of pg_gemm w.r.t. W / bias
 * (nn.Linear weight gradients). */
int pg_gemm_wgrad(const float* dY, int ldy, const float* X, int ldx, int M, int N, int K, float* gW, int ldgw,
                  float* gb, void* stream);

/* out[ctx(a)][0:ncol] (=) sum of Y[e][0:ncol] over the bond rows e whose source (by_src != 0) or target (by_src == 0) is ligand
 * atom a; rows of `out` are context nodes (pharmacophore rows are not written).  Adjoint of pg_gemm's gathered operand
 * add1[idx1[r]] with idx1 = PgTopo.bond_src / bond_dst (reference: the h_k / h_j columns of the concatenated first layers,
 * models/uni_denoiser.py:43-59,141-155,190-201).  ncol, ldy, ldo multiples of 4; rows 16-byte aligned. */
int pg_bond_rows_sum(const PgTopo* t, const float* Y, int ldy, int ncol, int by_src, float* out, int ldo, void* stream);

/* Y = ReLU(LayerNorm_128(X) * gamma + beta) and its adjoint (the LayerNorm+ReLU between the two Linear layers of
 * models/common.py:99-119 MLPs, used where the forward keeps it fused into pg_gemm's operand load).
 * gX (=), ggamma / gbeta (+=). */
int pg_ln_relu(const float* X, int ldx, const float* gamma, const float* beta, int M, float* Y, int ldy, void* stream);
int pg_ln_relu_bwd(const float* X, int ldx, const float* gamma, const float* beta, const float* gY, int ldgy, int M,
                   float* gX, int ldgx, float* ggamma, float* gbeta, void* stream);

/* adjoint of pg_seg_attn (same PgSegAttn inputs as the forward call, with U and Cdst_k/v given explicitly in every
 * mode; triplet: Cdst = smear(d_ji) . Wg2 computed by the caller, S/swn form) */
typedef struct {
  const float* gS; const float* gswn;     /* non-pos modes: gradient of S [..][32][64] and swn [..][16]            */
  const float* gdx;                        /* pos modes: gradient of dx [n_ctx,3]                                    */
  float* gU;                               /* (=) [..][32][64] lane-fixed, rows = segments                           */
  float* gCdst_k; float* gCdst_v; int ld_gcdst;   /* (=) rows = segments                                            */
  float* gCsrc_k; float* gCsrc_v; int ld_gcsrc;   /* (+=) rows as Csrc                                              */
  float* gWf_k; float* gWf_v;              /* (+=) lane-fixed [F/4][8][64]                                           */
  float* gbk; float* gbv;                  /* (+=) [128] gradient of b' = beta/|gamma| (PgSegAttn.ln_bk / ln_bv)     */
  float* gW2xv_l; float* gb2xv;            /* (+=) pos modes                                                         */
  float* gx; float* gnrm;                  /* (+=) [n_ctx,3]; NULL = not needed (pharmacophore encoder)              */
  float* gew;                              /* (=) knn modes [n_ctx,k]                                                */
  const float* alpha; int alpha_rows;      /* optional, from the forward (PgSegAttn.alpha): triplet / node-update modes: softmax weights
                                              [segments][alpha_rows][16]; position modes: logits | value scalars [..][alpha_rows][32] */
  const float* S; const float* swn;        /* ... with the forward's S / swn: one pass instead of two                */
  float* rowbuf; int rowbuf_rows; int grid;/* scratch: grid * pg_seg_attn_bwd_waves(mode) * rowbuf_rows * 48 floats,
                                              rowbuf_rows >= rows of the largest segment; grid = workgroups to launch */
  const int* atom_order;                   /* PG_SEG_TRIPLET, optional: [n_lig] ligand atoms (0 .. n_lig-1) in the order the persistent
                                              workgroups take them (workgroup b: entries b, b + grid, ...).  The kernel works off one SOURCE
                                              ATOM per workgroup round and an atom costs ~ (n-1) x ceil(n/16): in index order the slowest of
                                              256 workgroups carries 16 % more than the average on the config-5 batch; sorted by cost and
                                              dealt out in a snake it is 1 %.  NULL = index order.  Results do not depend on it. */
  float* dlogit; float* gfeat_v;           /* optional scratch, PG_SEG_TRIPLET (ligands up to 64 atoms), PG_SEG_KNN_NODE, PG_SEG_KNN_POS with the forward's
                                              per-row record (alpha) given: [segments][alpha_rows][16] and [segments][alpha_rows][16 * ceil(F / 16)]
                                              floats (F = 12 / 48 / 48).  With both, the adjoint runs as a value pass and a key pass (a wave holds ONE
                                              MLP path and fits 512 registers without spilling); the value pass leaves d logit (position update: one
                                              scalar per row) and its d feat rows there for the key pass.  Same gradients up to the order of the
                                              weight-gradient atomics. */
  int tri_form;                            /* PG_SEG_TRIPLET, ligands of up to 64 atoms, Cdst_v == Cdst_k + 128: 0 = one wave per 16-row tile
                                              (csrc/seg_attn_bwd.hip; the forms above); 1 / 2 = the channels of a tile split over the waves of a
                                              workgroup (csrc/triplet_bwd2.hip: nothing of the forward is read back -- alpha, S, swn, dlogit, gfeat_v,
                                              rowbuf unused; same gradients up to summation order): 1 = 4 waves x 32 channels, 2 = ligands of up to
                                              32 atoms on 8 waves x 16 channels and the larger ones in a second launch of the 4-wave form */
} PgSegAttnGrad;
int pg_seg_attn_bwd_waves(int mode);      /* the largest PgSegForm.rowbuf_waves of any form of the mode */
int pg_seg_attn_bwd(const PgTopo* t, const PgSegAttn* p, const PgSegAttnGrad* g, void* stream);
/* The form pg_seg_attn_bwd would run (see pg_seg_attn_form).  The form is inferred from what the caller filled in: alpha + S + swn
 * (the forward's record) select the one-pass kernels, dlogit + gfeat_v on top the two-pass form, tri_form the channel-split one. */
int pg_seg_attn_bwd_form(const PgTopo* t, const PgSegAttn* p, const PgSegAttnGrad* g, PgSegForm* out);

/* gW2_l (+=) in the lane-fixed layout of W2k_l / W2v_l:  gW2[8h+d, c] += sum_s X[s, 8h+d] * T[s][c][h]
 * (adjoint of pg_attn_fold_query w.r.t. the weights with X = q, T = dU; of pg_attn_unfold_value with X = dout, T = S) */
int pg_attn_fold_wgrad(const float* X, int ldx, const float* T, int n, const int* ids, float* gW2_l, void* stream);

/* the bias side of pg_attn_unfold_value's adjoint over the rows `ids` (NULL: all n):
 * gswn[s, h] (=) sum_d gout[s, 8h+d] * b2v[8h+d];  gb2v[c] (+=) sum_s gout[s, c] * swn[s, c >> 3]  (rows outside `ids`: untouched) */
int pg_attn_unfold_bias_grad(const float* gout, int ldg, const float* swn, const float* b2v, int n, const int* ids,
                             float* gswn /*[.,16]*/, float* gb2v /*[128]*/, void* stream);

/* ---- from sampler output to molecules (phoregen_amd/molecule.py; rule of utils/sample_utils.py:96-132, sample_all.py:79-175) ----
 * Screens F frames of a batch of B graphs, one wave per (frame, graph): atom class = argmax of 12 scores (class 11 = masked atom,
 * dropped; kept atoms are numbered in order), bond order of the pair a < b = argmax of 6 scores (1..4 bonds, 4 = aromatic; 0 and 5 no
 * bond; a bond with a dropped end is dropped), per kept atom degree and valence2 = sum of 2 x order (aromatic = 3), connected
 * components of the kept atoms (label = smallest local atom index of the component), and a status word.  First maximum wins (a NaN
 * score counts as the largest, as torch.argmax has it).  Only the FIRST half of a graph's bond rows is read: rows [0, n(n-1)/2) of a
 * graph with n atoms are the pairs a < b in row-major order (phoregen_amd/plan.py make_edge_data); g_bond_off counts both halves.
 * Scores are logits or one-hots, fp32, rows contiguous: frame f of node_scores starts at node_scores + f * node_fs ELEMENTS (likewise
 * edge_scores / pos; F = 1 with stride 0 for a single prediction).  node_scores and node_fs 16-byte, edge_scores and edge_fs 8-byte
 * aligned.  max_valence2 [11]: twice the largest explicit valence per atom class (one more is allowed to an atom with an aromatic bond).
 * max_n = the largest atom count of the batch: above PG_MOL_MAX_ATOMS, or with a negative size, the call returns an error before
 * anything is launched.
 * Every element of every output is written (nothing needs zeroing); integer work only, so results are exact.
 *   status [F][B], counts [F][B][4] = kept atoms, bonds, components, atoms of the largest component
 *   cls [F][n_lig] (-1 = dropped), compact [F][n_lig] (-1 = dropped), valence2 [F][n_lig] (saturates at 255), comp [F][n_lig] (-1 = dropped)
 *   order [F][n_bond / 2] (0..4; the rows of graph g start at g_bond_off[g] / 2) */
#define PG_MOL_MAX_ATOMS 128
#define PG_MOL_NO_ATOMS 1            /* failures: nothing kept ...                                             */
#define PG_MOL_DISCONNECTED 2        /* ... more than one component ...                                        */
#define PG_MOL_VALENCE 4             /* ... an atom above its largest valence ...                              */
#define PG_MOL_NONFINITE 8           /* ... a kept atom with a non-finite coordinate                           */
#define PG_MOL_HAD_MASKED_ATOM 16    /* informational: an atom of class 11 was dropped                         */
#define PG_MOL_HAD_ABSORBING_BOND 32 /* informational: a first-half bond row of class 5                        */
int pg_mol_screen(const float* node_scores, int64_t node_fs, const float* edge_scores, int64_t edge_fs, const float* pos,
                  int64_t pos_fs, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig,
                  int n_bond, int max_n, const uint8_t* max_valence2 /*[11]*/, int* status, int* counts, int8_t* cls,
                  int16_t* compact, uint8_t* valence2, int16_t* comp, int8_t* order, void* stream);

/* The same screen with the bonds perceived from the coordinates instead of the edge scores (phoregen_amd/molecule.py
 * screen(bonds='distance'); the rule of the reference's utils/predict_bonds.py, DESIGN.md 2.9 "Distance bonds").  Atom classes are
 * the argmax of node_scores as above.  For the pair a < b of two kept atoms whose coordinates are finite, with d100 = 100.0f *
 * sqrtf(dx*dx + dy*dy + dz*dz) in fp32 and t = thresholds[class a][class b]: order 0 unless d100 < t[0]; then 2 if d100 < t[1], and 3
 * if also d100 < t[2]; else 1.  All compares are strict, so an entry of 0 means "no such bond".  thresholds [11][11][3] fp32 (bond
 * length + margin in pm; the caller hands in a symmetric table).  Any other pair has order 0.  There is no aromatic order and no
 * absorbing class: PG_MOL_HAD_ABSORBING_BOND is never set.  PG_MOL_DIST_UNMAPPED_ELEMENT (informational) marks a graph with a kept atom
 * of class 0 (B) or 5 (Si), the two elements the reference's rule cannot name.  The seven outputs are pg_mol_screen's, in the same
 * layouts, every element written.
 * edge_scores may be NULL.  If not (edge_fs as above; only the first half of a graph's rows is read), agree [F][B][6] is written: over
 * the pairs a < b of kept atoms with finite coordinates, with p = the argmax of the pair's scores (0 and 5: no bond) and o = the
 * distance order, the number of pairs with p = o in 1..3; p = 4 and o in 1..2; both bonded otherwise; p only; o only; neither.
 * With edge_scores NULL agree is not touched.
 * node_scores and node_fs 16-byte, counts 16-byte, a non-null edge_scores and edge_fs 8-byte aligned.  max_n above PG_MOL_MAX_ATOMS,
 * a negative size, a null table, or edge_scores without agree: error before anything is launched, outputs untouched.  Compares and
 * integer counts only (no floating-point sum), so a graph's rows do not depend on its batch. */
#define PG_MOL_DIST_UNMAPPED_ELEMENT 64 /* informational: a kept B or Si atom                                  */
int pg_mol_screen_dist(const float* node_scores, int64_t node_fs, const float* pos, int64_t pos_fs, const float* edge_scores,
                       int64_t edge_fs, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig,
                       int n_bond, int max_n, const uint8_t* max_valence2 /*[11]*/, const float* thresholds /*[11][11][3]*/,
                       int* status, int* counts, int8_t* cls, int16_t* compact, uint8_t* valence2, int16_t* comp, int8_t* order,
                       int* agree /*[F][B][6]*/, void* stream);

/* Identity keys of the molecules the screen decoded, one wave per (frame, graph).  Reads the screen's outputs cls [F][n_lig] and
 * order [F][n_bond / 2] (frames are dense: frame f starts at f * n_lig / f * n_bond / 2) with the same offsets; an atom is kept if
 * its class is 0..10, a pair row is a bond if its order is 1..4 and both ends are kept.  key [F][B]: a 64-bit value that does not
 * depend on the numbering of the atoms (dropped atoms, their place in the row order, absorbing rows and the reversed half of the bond
 * rows have no influence); equal keys are necessary, not sufficient, for equal molecules.  colour [F][n_lig] (may be NULL): the final
 * refinement colour of every kept atom, 0 for a dropped one.  Definition (initial colour from class, valence2, degree and aromatic
 * bond count; three rounds over all atom pairs with hop distance and bond order; wrapping 64-bit sums): DESIGN.md 2.9.  A graph
 * without a kept atom has the key 0xE220A8397B1DCDAF.  max_n above PG_MOL_MAX_ATOMS or a negative size: error before anything is
 * launched, outputs untouched.  Every element of both outputs is written; integer work only, so results are exact. */
int pg_mol_key(const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
               int n_lig, int n_bond, int max_n, int64_t* key, int64_t* colour, void* stream);

/* Geometry and pharmacophore fit of the molecules the screen decoded, one wave per (frame, graph).  Reads the coordinates (pos, pos_fs
 * as pg_mol_screen takes them) and the screen's outputs cls [F][n_lig] and order [F][n_bond / 2] (frames dense) with the same offsets.
 * An atom is kept if its class is 0..10 and its three coordinates are finite; a kept-class atom with a non-finite coordinate sets
 * PG_GEOM_NONFINITE and is left out of everything else.  A pair a < b of kept atoms is bonded if its order is 1..4, else non-bonded.
 * Distance = sqrtf(dx*dx + dy*dy + dz*dz) in fp32 from fp32 differences.  Points: point_pos [n_point][3] in the coordinates of pos,
 * point_is_ex [n_point] (non-zero = exclusion sphere, else feature); graph g has the rows g_point_range[g][0] .. [g][1] (ranges may
 * coincide between graphs and may be empty) and writes its per-point outputs from g_point_out_off[g] on (g_point_out_off [B+1], the
 * running sum of the range lengths; n_point_out = its last entry).  A non-finite point sets PG_GEOM_NONFINITE too, has point_dist +inf
 * and point_atom -1, and is left out of everything else.  limits: five floats in HOST memory, read during the call: bond_min,
 * bond_max, clash_min, ex_clear, feat_cut; all comparisons are strict.
 *   point_dist [F][n_point_out], point_atom [F][n_point_out]: distance to the nearest kept atom and that atom's compact index (its
 *     index among the graph's atoms of class 0..10, as the screen's `compact`); first minimum in atom order; +inf and -1 without one
 *   metrics [F][B][8]: 0 min / 1 max bonded distance (+inf / -inf without a bond), 2 min non-bonded distance (+inf if none),
 *     3 min point_dist over exclusion spheres (+inf if none), 4 max point_dist over features (-inf if none), 5 |centroid of the kept
 *     atoms - mean of the features| (NaN if either is empty), 6 mean over bonds of max(d - bond_max, 0) + max(bond_min - d, 0)
 *     (0 without a bond), 7 = 0 (reserved).  5 and 6 are summed in fp64 from the fp32 inputs and rounded once.
 *   counts [F][B][6]: bonds with d < bond_min, bonds with d > bond_max, non-bonded pairs with d < clash_min, (atom, exclusion sphere)
 *     pairs with d < ex_clear, features with point_dist < feat_cut, features
 *   status [F][B]: PG_GEOM_* bits; the first four are set exactly when their count is non-zero, FEATURE_MISSED when covered < features
 * Sums are per-lane partials in a fixed lane-to-element assignment and a fixed butterfly, no floating-point atomics: a graph's row does
 * not depend on its batch.  max_n above PG_MOL_MAX_ATOMS or a negative size: error before anything is launched, outputs untouched.
 * Every element of every output is written (nothing needs zeroing). */
#define PG_GEOM_BOND_SHORT 1
#define PG_GEOM_BOND_LONG 2
#define PG_GEOM_CLASH 4
#define PG_GEOM_EX_CLASH 8
#define PG_GEOM_FEATURE_MISSED 16    /* informational: a feature without a kept atom inside feat_cut */
#define PG_GEOM_NONFINITE 32
int pg_mol_geom(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/,
                const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig, int n_bond, int max_n, const float* point_pos,
                const uint8_t* point_is_ex, int n_point, const int* g_point_range /*[B][2]*/, const int* g_point_out_off /*[B+1]*/,
                int n_point_out, const float* limits /*[5] host*/, float* point_dist, int16_t* point_atom, float* metrics, int* counts,
                int* status, void* stream);

/* Ring perception of the molecules the screen decoded, one wave per (frame, graph).  Reads the screen's outputs cls [F][n_lig] and
 * order [F][n_bond / 2] (frames dense) with the same offsets, as pg_mol_key does: an atom is kept if its class is 0..10, a pair row
 * a < b is a bond if its order is 1..4 and both ends are kept; degree = an atom's bonds.  Definition: DESIGN.md 2.9 "Rings".
 *   ring_size [F][n_bond / 2] (aligned with order): 1 + bonds on a shortest path between the bond's ends that does not use the bond,
 *     i.e. the atoms of the smallest ring through it; 0 for a bridge and for a pair that is no bond.  Ring bond: ring_size > 0.
 *   atom_ring [F][n_lig]: smallest ring_size among the atom's ring bonds; 0 for an atom without one or a dropped atom
 *   ring_sys [F][n_lig]: smallest local atom index reachable over ring bonds (rings that share an atom are one system); -1 likewise
 *   counts [F][B][PG_RING_N_COUNTS]: 0 rings = bonds - kept atoms + components, 1 ring bonds, 2 ring atoms, 3 ring systems, 4 smallest
 *     and 5 largest ring_size among ring bonds (0 without one), 6 atoms of the largest ring system, 7 rotatable = bonds of order 1 with
 *     ring_size 0 and both ends of degree >= 2, 8 bonds of order 4 with ring_size 0, 9 kept atoms with exactly one bond of order 4
 *   status [F][B]: PG_RING_* bits
 * limits: four ints in HOST memory, read during the call: ring_min, ring_max, system_max, rotatable_max.  Integer work only, counts are
 * per-lane partials in a fixed butterfly or integer LDS atomics: results are exact and a graph's rows do not depend on its batch.
 * max_n above PG_MOL_MAX_ATOMS, a negative size or null limits: error before anything is launched, outputs untouched.  Every element
 * of every output is written (nothing needs zeroing). */
#define PG_RING_AROMATIC_OUTSIDE 1   /* a bond of order 4 that is in no ring                                   */
#define PG_RING_SMALL 2              /* a ring bond whose smallest ring has fewer than limits.ring_min atoms   */
#define PG_RING_LARGE 4              /* ... more than limits.ring_max atoms                                    */
#define PG_RING_SYSTEM_LARGE 8       /* a ring system of more than limits.system_max atoms                     */
#define PG_RING_ROTATABLE 16         /* more than limits.rotatable_max rotatable bonds                         */
#define PG_RING_AROMATIC_LONE 32     /* informational: an atom with exactly one bond of order 4                */
#define PG_RING_N_COUNTS 10
int pg_mol_rings(const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
                 int n_lig, int n_bond, int max_n, const int* limits /*[4] host*/, uint8_t* ring_size, uint8_t* atom_ring,
                 int16_t* ring_sys, int* counts, int* status, void* stream);

/* Kekulé form, hydrogens and charges of the molecules the screen decoded, one wave per (frame, graph).  Reads the screen's outputs
 * cls [F][n_lig] and order [F][n_bond / 2] (frames dense) with the same offsets, as pg_mol_rings does: an atom is kept if its class is
 * 0..10, a pair row a < b is a bond if its order is 1..4 and both ends are kept.  Definition: DESIGN.md 2.9 "Kekulé form".  Per kept
 * atom a = its bonds of order 4, s = the sum of the orders of its other bonds; an atom with a >= 1 is aromatic and, in a pass with the
 * table `cap`, NOT (s + a + 1 > cap[class]), MUST (else, must[class] != 0) or MAY.  Pass 0: cap = dbl_neutral; pass 1, run only if
 * pass 0 is infeasible and allow_charged != 0: cap = max(dbl_neutral, dbl_charged).  A pass is feasible iff the bonds of order 4
 * between atoms that are not NOT have a matching that covers every MUST atom; the kernel returns such a matching of maximum
 * cardinality (Edmonds' algorithm with blossom contraction, exact; which maximum matching is not specified, its cardinality is).
 * d = 1 for a matched atom; v = s + a + d; q = 1 if (class is N and v == 4) or (d == 1 and v > dbl_neutral[class]), else 0;
 * h = t - (v - q) with t the smallest non-zero entry of h_valences[class] that is >= v - q, h = 0 without one.  If no pass is feasible
 * PG_KEKULE_FAILED is set, kekule_order = order and every d = 0.
 *   dbl_neutral, dbl_charged, must: uint8 [11] in DEVICE memory; h_valences: uint8 [11][4] in device memory, ascending, zero-padded
 *   kekule_order [F][n_bond / 2] (aligned with order): order with every bond of order 4 replaced by 2 (matched) or 1; other rows copied
 *   hcount [F][n_lig], charge [F][n_lig]: h and q per atom, 0 for a dropped atom
 *   counts [F][B][PG_KEKULE_N_COUNTS]: 0 aromatic atoms, 1 bonds of order 4, 2 doubled bonds (0 on failure), 3 MUST atoms, 4 matched
 *     MAY atoms (3 and 4 by the classification of the last pass run), 5 sum of h, 6 sum of q, 7 N or O atoms with h >= 1, 8 N and O
 *     atoms, 9 kept atoms
 *   status [F][B]: PG_KEKULE_* bits
 * Integer work only: results are exact, and a graph's rows, the matching included, do not depend on its batch.  max_n above
 * PG_MOL_MAX_ATOMS, a negative size or a null table: error before anything is launched, outputs untouched.  Every element of every
 * output is written (nothing needs zeroing). */
#define PG_KEKULE_FAILED 1           /* no feasible pass                                                       */
#define PG_KEKULE_CHARGED 2          /* informational: the matching is pass 1's (never together with FAILED)   */
#define PG_KEKULE_HAS_AROMATIC 4     /* informational: an atom with a bond of order 4                          */
#define PG_KEKULE_CATION 8           /* informational: an atom with q != 0                                     */
#define PG_KEKULE_N_COUNTS 10
int pg_mol_kekule(const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
                  int n_lig, int n_bond, int max_n, const uint8_t* dbl_neutral /*[11]*/, const uint8_t* dbl_charged /*[11]*/,
                  const uint8_t* must /*[11]*/, const uint8_t* h_valences /*[11][4]*/, int allow_charged, int8_t* kekule_order,
                  uint8_t* hcount, int8_t* charge, int* counts, int* status, void* stream);

/* Pharmacophore feature typing of the molecules the screen decoded and the typed match against their feature points, one wave per
 * (frame, graph).  Definition: DESIGN.md 2.9 "Features".  Reads the coordinates (pos, pos_fs as pg_mol_geom takes them), the screen's
 * cls [F][n_lig], order [F][n_bond / 2] and compact [F][n_lig], pg_mol_kekule's kekule_order [F][n_bond / 2], hcount, charge [F][n_lig]
 * and status [F][B], and pg_mol_rings' ring_size [F][n_bond / 2] (frames dense, the same offsets).  Every kept atom (class 0..10) gets
 * a byte with one bit per type, in the order HD, AR, PO, HA, HY, NE, XB (bit 0..6): the reference's SMARTS per type restated as
 * integer rules over element, hydrogens, charge, degree, Kekulé bond orders, the screen's aromatic bond class and ring membership
 * (csrc/feature_core.h).  A graph whose Kekulé status has PG_KEKULE_FAILED has all bytes 0 and PG_FEAT_NO_KEKULE.
 * Points: point_pos [n_point][3] in the coordinates of pos, point_kind int8 [n_point]: 0..6 = the type to match, -1 = a feature of a
 * type that is not typed (counted, never matched, never missed), anything else = ignored (exclusion spheres).  Graph g has the rows
 * g_point_range[g][0] .. [g][1] and writes its per-point outputs from g_point_out_off[g] on, as in pg_mol_geom.  A typed point of type
 * t is matched iff a kept atom with finite coordinates carries bit t and lies at a distance < feat_cut (strict; distance =
 * sqrtf(dx*dx + dy*dy + dz*dz) in fp32, as pg_mol_geom).  A kept atom or a typed or untyped point with a non-finite coordinate sets
 * PG_FEAT_NONFINITE; such an atom matches nothing, such a point is left out of every count.
 *   atom_fp [F][n_lig]: the byte; 0 for a dropped atom
 *   point_dist [F][n_point_out], point_atom [F][n_point_out]: distance to the nearest atom THAT CARRIES THE POINT'S TYPE and that
 *     atom's compact index; first minimum in atom order; +inf and -1 without one, and for every point that is not typed
 *   counts [F][B][PG_FEAT_N_COUNTS]: 0 typed points, 1 matched, 2 unmatched, 3 untyped points, 4..10 atoms per type, 11..17 points per
 *     type, 18..24 matched points per type
 *   status [F][B]: PG_FEAT_* bits; UNMATCHED iff unmatched > max_unmatched
 * Typing is integer work and exact; a graph's rows do not depend on its batch.  max_n above PG_MOL_MAX_ATOMS, a negative size or (with
 * B, F > 0) a null array: error before anything is launched, outputs untouched.  Every element of every output is written. */
#define PG_FEAT_NO_KEKULE 1          /* the graph has no Kekulé structure to type from                         */
#define PG_FEAT_UNMATCHED 2          /* more than max_unmatched typed points without a carrying atom in reach  */
#define PG_FEAT_HAS_UNTYPED 4        /* informational: a point of kind -1                                      */
#define PG_FEAT_NONFINITE 8          /* a kept atom or a point with a non-finite coordinate                    */
#define PG_FEAT_N_COUNTS 25
int pg_mol_feat(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int16_t* compact,
                const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge, const int* kekule_status /*[F][B]*/,
                const uint8_t* ring_size, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig,
                int n_bond, int max_n, const float* point_pos, const int8_t* point_kind, int n_point,
                const int* g_point_range /*[B][2]*/, const int* g_point_out_off /*[B+1]*/, int n_point_out, float feat_cut,
                int max_unmatched, uint8_t* atom_fp, float* point_dist, int16_t* point_atom, int* counts, int* status, void* stream);

/* SMILES text of the molecules the screen decoded, one wave per (frame, graph).  Definition: DESIGN.md 2.9 "SMILES".  Reads the screen's
 * cls [F][n_lig] and pg_mol_kekule's kekule_order [F][n_bond / 2], hcount, charge [F][n_lig] and status [F][B] (frames dense, the same
 * offsets): an atom is kept if its class is 0..10, a pair row a < b is a bond if its Kekulé order is 1, 2 or 3 and both ends are kept.
 * Depth-first from every kept atom not yet visited, ascending, neighbours ascending; a bond outside the tree is a ring closure, opened
 * at the ancestor with the smallest label 1..99 not in use and closed at the descendant; Kekulé form ('=' and '#', no aromatic
 * lower case), bracket atoms where the bare symbol would not read back with the atom's hydrogens and charge.  Not canonical.
 *   valences: uint8 [11][4] in DEVICE memory: the notation's normal valences per class, ascending, zero-padded; an empty row = the
 *     element is always bracketed
 *   text [F][B][capacity]: ASCII, every byte from length on 0; the whole row is written
 *   length [F][B]: bytes of text; 0 on a failing graph
 *   atom_rank [F][n_lig]: the atom's position in the text (preorder over the whole graph); -1 for a dropped atom and on a failing graph
 *   counts [F][B][PG_SMILES_N_COUNTS]: 0 bytes of text, 1 kept atoms, 2 bonds, 3 components, 4 ring closures, 5 '(' in the text,
 *     6 largest label (0: none), 7 bracket atoms; all 0 on a failing graph, except that with PG_SMILES_TOO_LONG they are the real ones
 *     and 0 is the bytes the text needs
 *   status [F][B]: PG_SMILES_* bits; with NO_KEKULE or RING_LABELS no other bit is set
 * Integer work only: results are exact, and a graph's rows do not depend on its batch.  max_n above PG_MOL_MAX_ATOMS, a negative size,
 * capacity < 1, a null table or (with B, F > 0) a null array: error before anything is launched, outputs untouched.  Every element of
 * every output is written (nothing needs zeroing). */
#define PG_SMILES_NO_KEKULE 1        /* failures: the graph's Kekulé status has PG_KEKULE_FAILED ...           */
#define PG_SMILES_RING_LABELS 2      /* ... more than 99 ring-closure labels would be in use at once ...       */
#define PG_SMILES_TOO_LONG 4         /* ... the text needs more than capacity bytes                            */
#define PG_SMILES_DISCONNECTED 8     /* informational: more than one component, the text has a '.'             */
#define PG_SMILES_EMPTY 16           /* informational: no kept atom, the text is empty                         */
#define PG_SMILES_BRACKET 32         /* informational: at least one bracket atom                               */
#define PG_SMILES_STEREO_DROPPED 64   /* informational, pg_mol_smiles_stereo: the marks of a group of double bonds contradicted each other and were left out */
#define PG_SMILES_N_COUNTS 8
#define PG_SMILES_N_STEREO_COUNTS 4
int pg_mol_smiles(const int8_t* cls, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                  const int* kekule_status /*[F][B]*/, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
                  int n_lig, int n_bond, int max_n, const uint8_t* valences /*[11][4]*/, int capacity, uint8_t* text, int* length,
                  int16_t* atom_rank, int* counts, int* status, void* stream);

/* Stereo perception of the molecules the screen decoded, one wave per (frame, graph).  Definition: DESIGN.md 2.9 "Stereo".  Reads the
 * coordinates (pos, pos_fs as pg_mol_geom takes them), the screen's cls [F][n_lig] and order [F][n_bond / 2], pg_mol_kekule's
 * kekule_order [F][n_bond / 2], hcount, charge [F][n_lig] and status [F][B], pg_mol_rings' ring_size [F][n_bond / 2] and pg_mol_key's
 * colour [F][n_lig] and key [F][B] (frames dense, the same offsets).  An atom is kept, a pair is a bond and degree is defined as in
 * pg_mol_rings; colours compare as unsigned 64-bit values; an implicit hydrogen is a ligand that differs from every heavy neighbour
 * and comes last in every ordering.
 * Centres: a candidate is an atom of class C, N, Si, P or S with (degree 4, no hydrogen) or (degree 3, one hydrogen); it is stereogenic
 * if its heavy neighbours have pairwise distinct colours.  With the neighbours n0 < n1 < n2 (< n3) in local index order, u_k the fp32
 * unit vector from the centre to n_k, and u3 = -(u0 + u1 + u2), not normalised, for the hydrogen: V = (u0 - u3) . ((u1 - u3) x (u2 - u3)).
 * Double bonds: a candidate is a pair a < b with Kekulé order 2, order != 4 and ring_size 0 whose ends each have no other bond of
 * Kekulé order >= 2 and either degree 3 or (degree 2 and at most one hydrogen); it is stereogenic if the two substituents (the
 * neighbours other than the partner) of every degree-3 end differ in colour.  With e = p_b - p_a, r_x the lowest-index substituent of
 * end x, d_x = p_r - p_x and w_x = d_x - e (d_x . e) / (e . e): t = (w_a . w_b) / (|d_a| |d_b|).
 *   atom_parity [F][n_lig]: 0 not stereogenic (or dropped); +1 / -1 the sign of V if |V| >= vol_min; 2 stereogenic but undefined:
 *     |V| < vol_min, a zero-length vector or a non-finite coordinate
 *   atom_label [F][n_lig]: atom_parity x the sign of the permutation that sorts the index-ordered ligands by ascending colour; 2 and 0
 *     stay.  It does not depend on the numbering of the atoms and flips under reflection.
 *   bond_stereo [F][n_bond / 2] (aligned with order): 0 not stereogenic (or no such bond); +1 cis, t >= planar_min; -1 trans,
 *     t <= -planar_min; 2 undefined
 *   bond_label [F][n_bond / 2]: bond_stereo, negated once for every end whose largest-colour substituent is not its lowest-index one
 *     (so for an end with one heavy substituent and a hydrogen); 2 and 0 stay
 *   stereo_key [F][B]: key if no element has label +1 or -1, else mix(key ^ mix(sum over such centres c of mix(colour[c] ^ (label > 0
 *     ? A : B)) + sum over such bonds of mix((mix(colour[a]) + mix(colour[b])) ^ (label > 0 ? C : D)))), wrapping sums, mix as in
 *     pg_mol_key, A .. D = 0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89
 *   counts [F][B][PG_STEREO_N_COUNTS]: centres 0 candidate, 1 stereogenic, 2 defined, 3 undefined; bonds 4 .. 7 likewise
 *   status [F][B]: PG_STEREO_* bits.  With NO_KEKULE every other output of the graph is 0 and stereo_key = key.
 * vol_min, planar_min: finite and above 0; max_undefined >= 0.  Perception is integer work on the colours and exact; the two
 * thresholds are compared in fp32.  A graph's rows do not depend on its batch.  max_n above PG_MOL_MAX_ATOMS, a negative size, a
 * threshold outside its range or (with B, F > 0) a null array: error before anything is launched, outputs untouched.  Every element
 * of every output is written (nothing needs zeroing). */
#define PG_STEREO_NO_KEKULE 1        /* the graph's Kekulé status has PG_KEKULE_FAILED: nothing to perceive from */
#define PG_STEREO_UNDEFINED 2        /* more than max_undefined stereogenic elements whose geometry does not decide */
#define PG_STEREO_HAS_CENTRE 4       /* informational: at least one centre with parity +1 or -1                */
#define PG_STEREO_HAS_BOND 8         /* informational: at least one double bond that is cis or trans           */
#define PG_STEREO_NONFINITE 16       /* a kept atom with a non-finite coordinate                               */
#define PG_STEREO_N_COUNTS 8
int pg_mol_stereo(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int8_t* kekule_order,
                  const uint8_t* hcount, const int8_t* charge, const int* kekule_status /*[F][B]*/, const uint8_t* ring_size,
                  const int64_t* colour, const int64_t* key /*[F][B]*/, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/,
                  int B, int F, int n_lig, int n_bond, int max_n, float vol_min, float planar_min, int max_undefined, int8_t* atom_parity,
                  int8_t* atom_label, int8_t* bond_stereo, int8_t* bond_label, int64_t* stereo_key, int* counts, int* status, void* stream);

/* pg_mol_smiles with the stereo of pg_mol_stereo in the text (isomeric SMILES).  Definition: DESIGN.md 2.9 "Stereo".  The arguments of
 * pg_mol_smiles and their meaning, traversal, labels, capacity, status bits and atom_rank included, plus atom_parity [F][n_lig] and
 * bond_stereo [F][n_bond / 2] (only the values +1 and -1 are read as stereo; with none of them the text is pg_mol_smiles's byte for byte).
 * Centres: an atom with parity +1 or -1 and (four bonds, no hydrogen) or (three bonds, one hydrogen) is a bracket atom '[', symbol, '@'
 * or '@@', 'H' with a hydrogen, '+' with a charge, ']'.  Its ligands stand in the text as: the parent, the hydrogen, the closures that
 * close at it by ascending ancestor, those that open at it by ascending descendant, the children ascending; '@' iff parity x the sign
 * of the permutation from index order (hydrogen last) to that order is +1 (parity +1: seen from the first ligand in index order the
 * others run counter-clockwise).  Double bonds: a pair with stereo +1 or -1 and Kekulé order 2 whose ends each have, besides the
 * partner, one or two neighbours, all joined by single bonds.  Every such single bond carries a mark, '/' = +1 or '\' = -1, written
 * where its bond symbol would stand (before the child, or before the opening label) and read from the atom written first to the atom
 * written later.  side(x, r) = the mark if x is written before r, else its opposite; the two substituents of an end have opposite
 * sides, and side(a, r_a) side(b, r_b) = bond_stereo for the lowest-index substituents.  Of the marked bonds joined by these rules
 * the one that comes first in the text is '/'.  If the rules contradict each other (never with pg_mol_stereo's output, whose stereo
 * double bonds are bridges) the marks of that group are left out and PG_SMILES_STEREO_DROPPED is set.
 *   stereo_counts [F][B][PG_SMILES_N_STEREO_COUNTS]: 0 centres written, 1 of them '@@', 2 marked bonds, 3 double bonds expressed; on a
 *     failing graph as counts
 * Errors as pg_mol_smiles; the three further arrays may not be null either. */
int pg_mol_smiles_stereo(const int8_t* cls, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                         const int* kekule_status /*[F][B]*/, const int8_t* atom_parity, const int8_t* bond_stereo,
                         const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig, int n_bond, int max_n,
                         const uint8_t* valences /*[11][4]*/, int capacity, uint8_t* text, int* length, int16_t* atom_rank, int* counts,
                         int* status, int* stereo_counts, void* stream);

/* Circular fingerprints of the molecules the screen decoded, one wave per (frame, graph).  Definition: DESIGN.md 2.9 "Fingerprints and
 * similarity".  Reads the screen's outputs cls [F][n_lig] and order [F][n_bond / 2] (frames dense) with the same offsets, exactly as
 * pg_mol_key does: an atom is kept if its class is 0..10, a pair row is a bond if its order is 1..4 and both ends are kept; aromatic
 * stays order 4 (no kekulisation).  With mix as in pg_mol_key: id_0[i] = mix(class | valence2 << 8 | degree << 24 | aromatic bonds
 * << 32), the key's initial colour; for r = 1 .. radius, id_r[i] = mix(id_(r-1)[i] ^ mix(sum over the bonds i - j of mix(id_(r-1)[j] ^
 * mix(order)))), sums wrapping at 64 bits.
 *   fp [F][B][PG_FP_WORDS]: bit (b & 63) of word (b >> 6) is set for b = id_r[i] & (PG_FP_BITS - 1), every kept atom i and every r in
 *     0 .. radius; all zero for a graph without a kept atom.  It does not depend on the numbering of the atoms, on dropped atoms,
 *     their place in the row order or absorbing rows.
 *   bits [F][B]: the set bits of the row
 * Not RDKit's ECFP (no duplicate-environment removal, other invariants, another hash).  0 <= radius <= PG_FP_MAX_RADIUS.  max_n above
 * PG_MOL_MAX_ATOMS, a negative size or a radius outside its range: error before anything is launched, outputs untouched.  Every word
 * of every row is written (nothing needs zeroing); integer work only, so results are exact. */
#define PG_FP_BITS 2048
#define PG_FP_WORDS 32
#define PG_FP_MAX_RADIUS 4
int pg_mol_fp(const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
              int n_lig, int n_bond, int max_n, int radius, uint64_t* fp /*[F*B*32]*/, int* bits /*[F*B]*/, void* stream);

/* Tanimoto similarity of fingerprint rows (PG_FP_WORDS 64-bit words each, 16-byte aligned).  For rows x, y: c = popcount(x & y),
 * u = popcount(x) + popcount(y) - c; sim = the fp32 value nearest to c / u (IEEE round to nearest even, whatever the build's
 * floating-point flags), and 1 if u = 0.  Popcounts are computed inside.  Every value is exact.
 *   out [na][nb]: sim(a_i, b_j).  na * nb above 2^31 - 1 is an error.
 * A negative size or a null pointer with a positive size: error before anything is launched. */
#define PG_FP_TILE_A 256             /* rows a workgroup holds in registers, one per lane ...                  */
#define PG_FP_TILE_B 64              /* ... and rows of one LDS tile of the other set                          */
int pg_fp_tanimoto(const uint64_t* a, int na, const uint64_t* b, int nb, float* out /*[na*nb]*/, void* stream);

/* For every row i of a against the rows j of b (no [na][nb] matrix in memory):
 *   sim [na]: the largest sim(a_i, b_j); index [na]: the lowest j that attains it; sum [na]: the fp64 sum over j of the fp32 values.
 * same != 0: a and b must be one set (one pointer, one size) and j = i is left out.  A row without a candidate (nb = 0, or same with
 * one row) gets sim -1, index -1, sum 0.  sim and index are exact and do not depend on how the work is cut; sum is added in a fixed
 * order for given sizes on a given device, within nb^2 * 2^-53 of the exact sum.  Where a has few rows and b many, b is cut into runs
 * that are combined in a second launch; their parts live in stream-ordered memory (hipMallocAsync), no host synchronisation. */
int pg_fp_nearest(const uint64_t* a, int na, const uint64_t* b, int nb, int same, float* sim /*[na]*/, int32_t* index /*[na]*/,
                  double* sum /*[na]*/, void* stream);

/* MaxMin diverse-subset picking over the n rows of fp: picked[0] = first, pick_sim[0] = -1; at step t >= 1 every unpicked row i has
 * m[i] = the largest sim to the rows picked so far, and the pick is the i with the smallest (m[i], i) in lexicographic order;
 * pick_sim[t] = that m[i].  A duplicate of a picked row has m = 1 and is picked last, lowest index first.  One launch per pick, each
 * reading the pick before it from slots and reducing into the next with a 64-bit atomicMin: no host synchronisation between picks.
 * work [n] and slots [k] are scratch the caller provides; their contents before and after the call mean nothing.  Exact.
 * k < 0, k > n, n < 0, first outside 0 .. n - 1 with n > 0, or a null array with k > 0: error before anything is launched. */
int pg_fp_maxmin(const uint64_t* fp, int n, int k, int first, int32_t* picked /*[k]*/, float* pick_sim /*[k]*/, float* work /*[n]*/,
                 uint64_t* slots /*[k]*/, void* stream);

/* Gaussian shape and feature ("colour") overlap of molecules where they lie, with no alignment.  Definition: DESIGN.md 2.9 "Shape".
 * A kept atom of class e is the Gaussian p exp(-alpha_e |r - x|^2), p = 2 sqrt(2).  For molecules A, B:
 *   V(A, B) = sum over kept atoms i of A, j of B of p^2 (pi / (a_i + a_j))^(3/2) exp(-(a_i a_j / (a_i + a_j)) d_ij^2)
 *   C(A, B) = sum over i, j of popcount(fp_i & fp_j) p^2 (pi / (2 a_c))^(3/2) exp(-(a_c / 2) d_ij^2), fp = the atoms' feature bytes
 *   ST = V(A, B) / (V(A, A) + V(B, B) - V(A, B)), CT the same over C; either is 0 where its denominator is not positive
 *   score = (1 - w) ST + w CT, each product and the sum rounded to fp32
 * fp32 arithmetic, first-order terms only, no hydrogens.  alpha: PG_SHAPE_N_ALPHA floats in HOST memory, the alpha of the 11 atom
 * classes, then the colour alpha a_c, in the units of the coordinates^-2; every entry point refuses an entry that is not positive and
 * finite.  A pair's values depend on the two molecules alone (one summation order per pair: csrc/shape_sim.hip), not on where they
 * sit in their sets, on the other rows, on the tiling or the split, or on which entry point computes them; V(A, B) and V(B, A) may
 * differ in the last bits.
 *
 * A set of n molecules is four arrays: atoms [n_atoms][4] fp32, 16-byte aligned (x, y, z, and as bits class | feature byte << 8, or
 * -1 for a dropped atom), mol [n][2] int32 (first atom row, atoms; at most PG_MOL_MAX_ATOMS; a row whose span leaves the atom rows
 * reads as empty), and the self overlaps self_shape [n], self_colour [n] = V(A, A), C(A, A).
 *
 * pg_shape_pack builds the set of F * B molecules in (frame, graph) order from a screen's cls [F][n_lig] and g_lig_off, the
 * coordinates pos (frame f at pos + f * pos_fs floats, rows of 3), the optional feature bytes atom_fp [F][n_lig] (null: all 0) and the
 * optional select [F * B] (uint8, null: all selected), one wave per molecule, no host read.  The kept atoms (class 0..10) of a graph
 * are compacted, in their order, to the front of the graph's span of atom rows, the rest of the span is written as dropped:
 * atoms [F * n_lig][4], mol [F * B][2], status [F * B] = PG_SHAPE_EMPTY (no kept atom) | PG_SHAPE_NONFINITE (a kept atom with a
 * non-finite coordinate) | PG_SHAPE_UNSELECTED.  A molecule with any bit has no atoms: an empty row.  Every element of the three
 * outputs is written.  max_n = the largest graph.
 * Errors, before anything is launched and with the outputs untouched: a negative size, max_n above PG_MOL_MAX_ATOMS, a null array
 * that is needed, a bad alpha. */
#define PG_SHAPE_N_ALPHA 12
#define PG_SHAPE_EMPTY 1
#define PG_SHAPE_NONFINITE 2
#define PG_SHAPE_UNSELECTED 4
#define PG_SHAPE_TILE_A 16           /* rows of set a per workgroup, one pair of molecules per wave at a time ... */
#define PG_SHAPE_TILE_B 16           /* ... and molecules of one LDS tile of set b; a run of b is whole tiles     */
int pg_shape_pack(const int8_t* cls, const int* g_lig_off /*[B+1]*/, const float* pos, int64_t pos_fs, const uint8_t* atom_fp,
                  const uint8_t* select, int B, int F, int n_lig, int max_n, const float* alpha /*host [12]*/,
                  float* atoms /*[F*n_lig*4]*/, int* mol /*[F*B*2]*/, int* status /*[F*B]*/, void* stream);

/* self_shape [n] = V(A, A) and, where self_colour is not null, self_colour [n] = C(A, A) of every row of a set (the terms i = j
 * included); one wave per row.  Errors as above. */
int pg_shape_self(const float* atoms, int n_atoms, const int* mol, int n, const float* alpha /*host [12]*/, float* self_shape /*[n]*/,
                  float* self_colour /*[n] or null*/, void* stream);

/* shape_out [na][nb] = ST(a_i, b_j) and, where colour_out is not null, colour_out [na][nb] = CT(a_i, b_j) (the self_colour arrays are
 * then read).  na * nb above 2^31 - 1 is an error.  Errors as above. */
int pg_shape_similarity(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape, const float* a_self_colour,
                        int na, const float* b_atoms, int b_n_atoms, const int* b_mol, const float* b_self_shape,
                        const float* b_self_colour, int nb, const float* alpha /*host [12]*/, float* shape_out /*[na*nb]*/,
                        float* colour_out /*[na*nb] or null*/, void* stream);

/* For every row i of a against the rows j of b (no [na][nb] matrix in memory), with the score above (has_colour = 0: CT = 0 and the
 * self_colour arrays are not read):
 *   sim [na]: the largest score; index [na]: the lowest j that attains it; sum [na]: the fp64 sum over j of the fp32 scores, j
 *   ascending within a run, the runs in their order.
 * same != 0: a and b must be one set (one mol pointer, one size) and j = i is left out.  An empty row of b scores 0 and is still a
 * candidate.  A row without a candidate (nb = 0, or same with one row) gets sim -1, index -1, sum 0.  sim and index do not depend on
 * how b is cut into runs; where a has few rows and b many, the runs are combined by a second launch in run order, their parts in
 * stream-ordered memory: no host synchronisation.  w outside [0, 1] or not a number is an error; errors as above. */
int pg_shape_nearest(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape, const float* a_self_colour,
                     int na, const float* b_atoms, int b_n_atoms, const int* b_mol, const float* b_self_shape,
                     const float* b_self_colour, int nb, int same, int has_colour, float w, const float* alpha /*host [12]*/,
                     float* sim /*[na]*/, int32_t* index /*[na]*/, double* sum /*[na]*/, void* stream);

/* Rigid overlay of molecule pairs: the best of up to five local ascents of the score above over the rigid poses of B, A fixed.
 * Definition: DESIGN.md 2.9 "Shape alignment".  A pose is (R, p): B's atom y lies at R (y - c_B) + p, c_B = B's centroid.
 *   frame of a row (pg_shape_frames, frames [n][PG_SHAPE_FRAME_FLOATS]): centroid 3 (the unweighted mean of the kept atoms), axes 9
 *     (axis k at 3 + 3 k: the eigenvectors of the covariance, divided by n, by cyclic Jacobi in double, eigenvalues descending, the
 *     largest-magnitude component of axes 1 and 2 positive, axis 3 = axis 1 x axis 2), rho = max(radius of gyration, 0.5), the three
 *     eigenvalues; computed in double in packed order and rounded once to fp32.  An empty row: origin, identity, rho 0.5, zeros.
 *   starts: 0 in place (R = I, p = c_B; B is read as stored until the first accepted step), 1..4 inertial (R = E_A D_k E_B^T,
 *     p = c_A, D_k = diag(1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1)); `starts` is a mask of the bits 0..4
 *     (PG_SHAPE_ALIGN_IN_PLACE, PG_SHAPE_ALIGN_INERTIAL).
 *   objective f = score(ST, CT, w) over V(A, B'), C(A, B') and the stored self overlaps; has_colour = 0 or w = 0: CT = C = 0 and the
 *     colour terms are skipped.  Gradient: force F = sum_ij 2 k_ij g_ij (x_i - y'_j), torque tau about p, each objective weighted by
 *     its chain-rule factor ((1 - w) (aa + bb) / (aa + bb - V)^2, w (caa + cbb) / (caa + cbb - C)^2, 0 for a denominator <= 0).
 *   step rule: d = g6 / |g6|, g6 = (F, tau / rho_B); trial p + s d[0:3], exp([s d[3:6] / rho_B]x) R (a unit quaternion, renormalised);
 *     f_trial > f: accept, s *= 1.5; else s *= 0.5; stop at |g6| = 0, s < min_step or after max_steps evaluations (the first counts).
 *   winner: the start with the largest final f, ties to the lowest start.
 * Outputs per pair: values [n_pairs][5] = V, C, ST, CT, score at the winning pose; transform [n_pairs][12] = R row-major, then
 * t = p - R c_B (y' = R y + t on B's stored coordinates); start [n_pairs]; steps [n_pairs] = the evaluations the winner used.  A
 * pair with an empty row: zeros, R = I, t = 0, start -1, steps 0.  A pair's outputs depend on the two rows and the arguments alone
 * (one summation order per evaluation: csrc/shape_align.hip).  pairs [n_pairs][2] int32 on the device names (row of a, row of b);
 * pairs = null: the grid a x b in row-major order, n_pairs = na * nb.  One workgroup per pair, one wave per start.
 * Errors, before anything is launched and with the outputs untouched: null arrays, negative sizes, a listed pair outside its set
 * (the list is read back once for this -- the one host read; the grid needs none), max_steps outside 1 .. PG_SHAPE_ALIGN_MAX_STEPS,
 * a step that is not positive and finite or min_step > first_step, an empty or unknown starts mask, w outside [0, 1] or not a
 * number, a bad alpha.  n_pairs = 0 is nothing to do. */
#define PG_SHAPE_FRAME_FLOATS 16
#define PG_SHAPE_ALIGN_N_STARTS 5
#define PG_SHAPE_ALIGN_IN_PLACE 0x01
#define PG_SHAPE_ALIGN_INERTIAL 0x1e
#define PG_SHAPE_ALIGN_MAX_STEPS 1024
int pg_shape_frames(const float* atoms, int n_atoms, const int* mol, int n, float* frames /*[n][16]*/, void* stream);
int pg_shape_align(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape, const float* a_self_colour,
                   const float* a_frames, int na, const float* b_atoms, int b_n_atoms, const int* b_mol, const float* b_self_shape,
                   const float* b_self_colour, const float* b_frames, int nb, const int32_t* pairs /*[n_pairs][2] or null*/, int n_pairs,
                   int has_colour, float w, const float* alpha /*host [12]*/, int max_steps, float first_step, float min_step, int starts,
                   float* values /*[n_pairs][5]*/, float* transform /*[n_pairs][12]*/, int32_t* start /*[n_pairs]*/,
                   int32_t* steps /*[n_pairs]*/, void* stream);

/* Substructure search: for every (frame, graph) the screen decoded and every pattern of a table, the embeddings of the pattern in the
 * molecule, one wave per (frame, graph, pattern).  Definition: DESIGN.md 2.9 "Substructure".
 * Target: the kept atoms (class 0..10) in the screen's compact numbering (compact [F][n_lig]) and the pair rows a < b with order 1..4
 * whose two ends are kept; order 4 (aromatic) is its own order.  An atom's properties: its class, its degree (kept bonds), hcount and
 * charge (pg_mol_kekule's), in a ring (atom_ring > 0), aromatic (it has a bond of order 4); a bond's: its order and whether it is a
 * ring bond (ring_size > 0).  ring_size [F][n_bond / 2] and atom_ring [F][n_lig] are pg_mol_rings' outputs, hcount, charge [F][n_lig]
 * and kekule_status [F][B] pg_mol_kekule's.
 * Pattern: a connected graph of 1 <= k <= PG_SUB_MAX_ATOMS query atoms, one table row of PG_SUB_PATTERN_BYTES bytes:
 *   PG_SUB_OFF_K       1 byte   k
 *   PG_SUB_OFF_MIN     int32    (little endian) the lower bound on `anchors`, >= 0
 *   PG_SUB_OFF_MAX     int32    the upper bound, -1 = none
 *   PG_SUB_OFF_ORDER   16 bytes the matching order: the query atom at position d, a permutation of 0 .. k - 1 that starts with atom
 *                               0 (the anchor) in which every later atom has a bond to an earlier one
 *   PG_SUB_OFF_ATOMS   16 records of PG_SUB_ATOM_BYTES bytes, query atom q at q: the element set as 11 bits (2 bytes, little endian),
 *                               degree lo, hi, hcount lo, hi (a byte each, inclusive; 0, 255 = any), flags = charge | ring << 2 |
 *                               aromatic << 4 with PG_SUB_ANY / PG_SUB_YES / PG_SUB_NO each (charge: YES = +1, NO = 0), one byte 0
 *   PG_SUB_OFF_BONDS   16 x 16 bytes, symmetric, byte [a][b] = 0 for no query bond, else the accepted orders as bits 0..3 (order o is
 *                               bit o - 1) | ring << 4 (PG_SUB_YES: a ring bond, PG_SUB_NO: a bridge)
 * Bytes that belong to atoms beyond k are not read.  An embedding is an injective map of the query atoms to kept atoms with every
 * atom record met at its image and every query bond on a target bond of an accepted order and ring flag; further target bonds between
 * images are allowed (a monomorphism).  A pattern that constrains hcount or charge has no embedding on a graph whose kekule_status
 * has bit 1 (failed) and gets PG_SUB_NO_KEKULE; other patterns do not read hcount, charge or kekule_status.
 * Outputs, frames dense, [F][B][P] plus the trailing dimension; every element is written:
 *   embeddings  the number of embeddings, saturating at 2^31 - 1
 *   anchors     the number of distinct atoms that are the image of query atom 0 in an embedding
 *   atom_mask   [2] bit c of word c >> 6: the atom with compact index c is in the image of an embedding
 *   first       [PG_SUB_MAX_ATOMS] the embedding whose images, listed in matching order, are lexicographically smallest, per query
 *               atom in the table's atom order; -1 beyond k, all -1 without an embedding
 *   status      PG_SUB_* bits; PG_SUB_OUT_OF_BOUNDS: anchors outside [min, max], or the row has a bound (min > 0 or max >= 0) and
 *               PG_SUB_TRUNCATED is set
 * Work bound: a step is one way to go on along the matching order: a partial embedding (the first d - 1 >= 1 query atoms of the order
 * mapped with every constraint among them met) and an unused atom that meets the d-th query atom's record and is joined to the image
 * of its walk parent (the earliest atom of the order it has a bond to) by a bond that query bond accepts; its other bonds to earlier
 * atoms are tested afterwards.  steps(r) = the number of steps whose anchor is the atom r.  A root with
 * steps(r) > max_steps is abandoned and PG_SUB_TRUNCATED set; then embeddings and anchors are lower bounds, atom_mask a subset and
 * first some embedding or -1.  Without the bit every output is exact.  1 <= max_steps <= PG_SUB_MAX_STEPS.
 * table [P][PG_SUB_PATTERN_BYTES] is device memory, table_host the same bytes in host memory: the rows are checked from it before
 * anything is launched (the library does not synchronise).  1 <= P <= PG_SUB_MAX_PATTERNS; F * B * P must fit one launch.
 * max_n above PG_MOL_MAX_ATOMS, a negative size, P or max_steps out of range, a malformed row (k outside 1..16, an empty element or
 * order set, lo > hi, a flag outside any / yes / no, an asymmetric bond byte, an order that is no such permutation, bad bounds) or a
 * null array with B, F > 0: error before anything is launched, outputs untouched.  Integer work only, so results are exact. */
#define PG_SUB_MAX_ATOMS 16
#define PG_SUB_MAX_PATTERNS 256
#define PG_SUB_MAX_STEPS 1073741824
#define PG_SUB_PATTERN_BYTES 416
#define PG_SUB_OFF_K 0
#define PG_SUB_OFF_MIN 4
#define PG_SUB_OFF_MAX 8
#define PG_SUB_OFF_ORDER 16
#define PG_SUB_OFF_ATOMS 32
#define PG_SUB_OFF_BONDS 160
#define PG_SUB_ATOM_BYTES 8
#define PG_SUB_ATOM_ELEMENTS 0
#define PG_SUB_ATOM_DEGREE 2
#define PG_SUB_ATOM_HCOUNT 4
#define PG_SUB_ATOM_FLAGS 6
#define PG_SUB_ANY 0
#define PG_SUB_YES 1
#define PG_SUB_NO 2
#define PG_SUB_MATCHED 1
#define PG_SUB_NO_KEKULE 2
#define PG_SUB_TRUNCATED 4
#define PG_SUB_OUT_OF_BOUNDS 8
int pg_mol_sub(const int8_t* cls, const int8_t* order, const int16_t* compact, const uint8_t* ring_size, const uint8_t* atom_ring,
               const uint8_t* hcount, const int8_t* charge, const int* kekule_status /*[F][B]*/, const int* g_lig_off /*[B+1]*/,
               const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig, int n_bond, int max_n, const uint8_t* table /*device*/,
               const uint8_t* table_host, int P, int max_steps, int* embeddings /*[F*B*P]*/, int* anchors /*[F*B*P]*/,
               int64_t* atom_mask /*[F*B*P*2]*/, int16_t* first /*[F*B*P*16]*/, int* status /*[F*B*P]*/, void* stream);

/* 3D positions for the hydrogens pg_mol_kekule counted, one wave per (frame, graph).  Definition: DESIGN.md 2.9 "Hydrogens".  Reads the
 * coordinates (pos, pos_fs as pg_mol_geom takes them), the screen's cls [F][n_lig] and order [F][n_bond / 2] and pg_mol_kekule's
 * kekule_order [F][n_bond / 2], hcount, charge [F][n_lig] and status [F][B] (frames dense, the same offsets; charge is not read: the
 * hydrogen count already carries it).  An atom is kept if its class is 0..10; its heavy neighbours are the kept atoms joined to it by a
 * pair row of Kekulé order 1..3, in ascending local index, d of them; u_k is the fp32 unit vector to the k-th.
 * A site is a kept atom with 1 <= hcount <= PG_HYD_MAX_PER_ATOM and finite coordinates at it and at every heavy neighbour.  Its shape:
 * linear if it has a bond of Kekulé order 3 or two of order 2; else trigonal if it has a bond of Kekulé order 2 or of the screen's
 * order 4, or is class N with d + hcount = 3 and a heavy neighbour that has such a bond; else tetrahedral.  Hydrogen k stands at
 * p + xh_length[class] * dir_k, dir_k by (shape, d, hcount) as DESIGN.md tabulates: opposite the neighbours' sum (3, 1), astride
 * it (tetrahedral 2, 1..2), on the cone around the one bond with the torsion set by the neighbour's lowest-index other neighbour or, without
 * one, by the coordinate axis most across the bond, negated for the higher of the two atoms (d = 1), the fixed vertices (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1) / sqrt(3)
 * (d = 0).  Every other combination, a neighbour at zero or non-finite distance (it is left out) and a vector to normalise with squared norm below
 * PG_HYD_DEG_EPS^2 take the generic rule: the first hydrogen opposite the neighbours' sum if that has a direction, every further one on
 * the fixed vertex whose largest dot product with the directions so far is smallest, first minimum.
 *   h_pos [F][n_lig][PG_HYD_MAX_PER_ATOM][3]: the hydrogens of the atom row, slot by slot; unused slots 0.  16-byte aligned.
 *   h_placed [F][n_lig]: the hydrogens placed at the atom, 0 or its hcount
 *   site_shape [F][n_lig]: 0 no site, else PG_HYD_SHAPE_* of the rule that placed them
 *   min_contact [F][B]: the smallest distance of a hydrogen to a kept atom other than its parent or to a hydrogen of another parent, fp32
 *     sqrtf of the squared distance as in pg_mol_geom; +inf without such a pair
 *   counts [F][B][PG_HYD_N_COUNTS]: 0 hydrogens placed, 1 sites, 2 .. 5 sites per shape (tetrahedral, trigonal, linear, generic), 6
 *     contacts: the pairs above closer than clash_min (strict), 7 kept atoms
 *   status [F][B]: PG_HYD_* bits.  With NO_KEKULE every other output of the graph is 0; with TOO_MANY (a kept atom with more than
 *     PG_HYD_MAX_PER_ATOM hydrogens) nothing is placed in the graph.
 * xh_length [11] is device memory, in class order; the library does not read it on the host, so the caller answers for finite lengths
 * of at least 0 (phoregen_amd.hydrogens.HydrogenOptions checks them).  A graph's rows do not depend on its batch.  max_n above
 * PG_MOL_MAX_ATOMS, a negative size, clash_min not finite or below 0, max_contacts below 0, a null table, a misaligned h_pos or (with
 * B, F > 0) a null array that has elements: error before anything is launched, outputs untouched.  Every element of every output is written (nothing
 * needs zeroing). */
#define PG_HYD_NO_KEKULE 1           /* the graph's Kekulé status has PG_KEKULE_FAILED: no hydrogen counts to place */
#define PG_HYD_NONFINITE 2           /* a kept atom with a non-finite coordinate: nothing placed at or next to it   */
#define PG_HYD_TOO_MANY 4            /* a kept atom with more than PG_HYD_MAX_PER_ATOM hydrogens                   */
#define PG_HYD_CONTACTS 8            /* more than max_contacts contacts                                        */
#define PG_HYD_GENERIC 16            /* informational: at least one site placed by the generic rule            */
#define PG_HYD_HAS_HYDROGEN 32       /* informational: at least one hydrogen placed                            */
#define PG_HYD_N_COUNTS 8
#define PG_HYD_MAX_PER_ATOM 4
#define PG_HYD_SHAPE_TETRAHEDRAL 1
#define PG_HYD_SHAPE_TRIGONAL 2
#define PG_HYD_SHAPE_LINEAR 3
#define PG_HYD_SHAPE_GENERIC 4
#define PG_HYD_DEG_EPS 1e-3f
int pg_mol_hydrogens(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int8_t* kekule_order,
                     const uint8_t* hcount, const int8_t* charge, const int* kekule_status /*[F][B]*/, const int* g_lig_off /*[B+1]*/,
                     const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig, int n_bond, int max_n, const float* xh_length /*[11] device*/,
                     float clash_min, int max_contacts, float* h_pos /*[F][n_lig][4][3]*/, uint8_t* h_placed /*[F][n_lig]*/,
                     uint8_t* site_shape /*[F][n_lig]*/, float* min_contact /*[F][B]*/, int* counts /*[F][B][PG_HYD_N_COUNTS]*/,
                     int* status /*[F][B]*/, void* stream);

/* Murcko scaffold of the molecules the screen decoded, written as the arrays of a screen of its own, one wave per (frame, graph).
 * Reads the screen's outputs cls [F][n_lig] and order [F][n_bond / 2] (frames dense) with the same offsets, as pg_mol_rings does: an
 * atom is kept if its class is 0..10, a pair row a < b is a bond if its order is 1..4 and both ends are kept.
 * Definition: DESIGN.md 2.9 "Scaffolds".  Core: what is left after every atom with at most one remaining neighbour has been removed,
 * again and again.  A bond of the core is a ring bond if a ring passes through it (pg_mol_rings' search), else a linker bond; an atom of the core with a
 * ring bond is a ring atom, any other a linker atom.  With PG_SCAF_EXOCYCLIC an atom outside the core that has a bond of order exactly
 * 2 to an atom of the core is kept as well (nothing else of it).  With PG_SCAF_GENERIC every scaffold atom gets carbon's class and
 * every scaffold bond order 1, after the selection.
 *   part [F][n_lig]: PG_SCAF_PART_* of the atom
 *   counts [F][B][PG_SCAF_N_COUNTS]: 0 scaffold atoms, 1 scaffold bonds, 2 ring atoms, 3 linker atoms, 4 exocyclic atoms, 5 side-chain
 *     atoms, 6 ring systems = components of the ring atoms under ring bonds, 7 linker bonds
 *   s_cls, s_compact, s_valence2, s_comp [F][n_lig], s_order [F][n_bond / 2], s_counts [F][B][4], s_status [F][B]: the scaffold as
 *     pg_mol_screen would write it had it decoded the scaffold alone: class (or carbon's) of a scaffold atom, else -1; index among the
 *     graph's scaffold atoms, else -1; twice the valence over scaffold bonds (aromatic 3), saturating at 255; smallest local index of
 *     the atom's scaffold component, else -1; order (or 1) of a bond between two scaffold atoms, else 0; scaffold atoms, bonds,
 *     components, atoms of the largest component; PG_MOL_NO_ATOMS (no scaffold atom) and PG_MOL_DISCONNECTED only: no valence rule.
 * The outputs must not overlap the inputs.  Integer work only: results are exact and a graph's rows do not depend on its batch or on
 * the numbering of its atoms (part, s_cls, s_valence2 move with the atoms).  max_n above PG_MOL_MAX_ATOMS, a negative size or flags
 * outside 0..3: error before anything is launched, outputs untouched.  Every element of every output is written (nothing needs
 * zeroing). */
#define PG_SCAF_EXOCYCLIC 1          /* flags: keep atoms double-bonded to the core                            */
#define PG_SCAF_GENERIC 2            /* flags: carbon's class and order 1 throughout the scaffold              */
#define PG_SCAF_PART_NONE 0          /* a dropped atom                                                         */
#define PG_SCAF_PART_SIDE_CHAIN 1
#define PG_SCAF_PART_LINKER 2
#define PG_SCAF_PART_RING 3
#define PG_SCAF_PART_EXOCYCLIC 4
#define PG_SCAF_CARBON 1             /* carbon's atom class                                                    */
#define PG_SCAF_N_COUNTS 8
int pg_mol_scaffold(const int8_t* cls, const int8_t* order, const int* g_lig_off /*[B+1]*/, const int* g_bond_off /*[B+1]*/, int B, int F,
                    int n_lig, int n_bond, int max_n, int flags, uint8_t* part /*[F][n_lig]*/, int* counts /*[F][B][PG_SCAF_N_COUNTS]*/,
                    int* s_status /*[F][B]*/, int* s_counts /*[F][B][4]*/, int8_t* s_cls, int16_t* s_compact, uint8_t* s_valence2,
                    int16_t* s_comp, int8_t* s_order /*[F][n_bond / 2]*/, void* stream);

/* Property descriptors and drug-likeness limits of the molecules the screen decoded, one wave per (frame, graph).  Reads the screen's
 * cls [F][n_lig] and order [F][n_bond / 2], the Kekulé form's kekule_order, hcount, charge and status [F][B], and the rings' ring_size
 * [F][n_bond / 2] and atom_ring [F][n_lig] (frames dense); no coordinates.  Definition: DESIGN.md 2.9 "Properties"; the rules are
 * csrc/props_core.h.  A "non-aromatic double bond" is a bond of Kekulé order 2 whose screen order is not 4, a "single bond" one of
 * Kekulé order 1 whose screen order is not 4.
 *   atom_env [F][n_lig]: the environment word of a kept atom (the PG_PROP_ENV_* fields, bits 30 and 31 are 0); -1 for a dropped atom
 *     and for every atom of a graph whose Kekulé status has PG_KEKULE_FAILED
 *   tables: n_tables <= PG_PROP_MAX_TABLES contribution tables, table t of table_rows[t] <= PG_PROP_MAX_ROWS rows, one after the other
 *     in device memory; a row is PG_PROP_ROW_INTS int32: mask, value, atom, per_h.  A kept atom takes the first row of a table with
 *     (env & mask) == value and adds atom + hcount * per_h to the graph's sum of that table; without such a row it adds 0 and counts as
 *     untyped.  The caller answers for |atom|, |per_h| < 2^20 (phoregen_amd.properties.PropertyTable checks them): then no sum of a
 *     graph of PG_MOL_MAX_ATOMS atoms leaves int32.
 *   atom_row [F][PG_PROP_MAX_TABLES][n_lig]: the row taken, 255 = none, an unused table or a dropped atom
 *   sums [F][B][PG_PROP_MAX_TABLES]: unused tables 0
 *   counts [F][B][PG_PROP_N_COUNTS]: the PG_PROP_C_* columns
 *   weights [PG_PROP_N_WEIGHTS] (device): the weight of an atom of class 0..10 and, last, of a hydrogen, times 1000
 *   weight_milli [F][B]: the sum of them over the kept atoms and their hydrogens
 *   limits [PG_PROP_N_LIMITS][2] (host): lo, hi per limited quantity in the order of the PG_PROP_L_* (INT_MIN / INT_MAX: none); a
 *     quantity below lo or above hi sets its bit in violated [F][B]
 *   status [F][B]: PG_PROP_* bits; PG_PROP_LIMITS with more set bits in `violated` than max_violations.  With PG_PROP_NO_KEKULE the
 *     counts, sums, weight and `violated` of the graph are 0, its rows 255, its words -1, and no limit is looked at.
 * Integer work only: results are exact, a graph's rows do not depend on its batch, and counts, sums and weight not on the numbering of
 * its atoms.  max_n above PG_MOL_MAX_ATOMS, a negative size, more than PG_PROP_MAX_TABLES tables, a table above PG_PROP_MAX_ROWS rows,
 * max_violations below 0 or (with B, F > 0) a null array: error before anything is launched, outputs untouched.
 * Every element of every output is written (nothing needs zeroing). */
#define PG_PROP_MAX_ROWS 128
#define PG_PROP_MAX_TABLES 4
#define PG_PROP_ROW_INTS 4
#define PG_PROP_N_WEIGHTS 12
#define PG_PROP_NO_KEKULE 1          /* the graph has no Kekulé structure to type from                         */
#define PG_PROP_LIMITS 2             /* more violated quantities than max_violations                           */
#define PG_PROP_UNTYPED 4            /* informational: an atom without a row in a table                        */
/* the word: shift of every field (widths: el 4, h 3, deg 3, n_dbl 2, nb_het 3, nb_arom 2, nb_hal 2, nb_no 3, every other 1) */
#define PG_PROP_ENV_EL 0
#define PG_PROP_ENV_H 4
#define PG_PROP_ENV_Q 7
#define PG_PROP_ENV_DEG 8
#define PG_PROP_ENV_AROM 11
#define PG_PROP_ENV_N_DBL 12
#define PG_PROP_ENV_TRIPLE 14
#define PG_PROP_ENV_RING 15
#define PG_PROP_ENV_RING3 16
#define PG_PROP_ENV_NB_HET 17
#define PG_PROP_ENV_NB_AROM 20
#define PG_PROP_ENV_DBL_O 22
#define PG_PROP_ENV_DBL_HET 23
#define PG_PROP_ENV_NB_DBL_HET 24
#define PG_PROP_ENV_NB_HAL 25
#define PG_PROP_ENV_NB_NO 27
/* the count columns */
#define PG_PROP_C_HEAVY_ATOMS 0
#define PG_PROP_C_HYDROGENS 1
#define PG_PROP_C_CARBONS 2
#define PG_PROP_C_SP3_CARBONS 3
#define PG_PROP_C_HETEROATOMS 4
#define PG_PROP_C_HALOGENS 5
#define PG_PROP_C_NHOH 6
#define PG_PROP_C_NO_COUNT 7
#define PG_PROP_C_ROTATABLE 8
#define PG_PROP_C_AMIDE_BONDS 9
#define PG_PROP_C_AROMATIC_ATOMS 10
#define PG_PROP_C_RING_ATOMS 11
#define PG_PROP_C_NET_CHARGE 12
#define PG_PROP_C_UNTYPED 13
#define PG_PROP_C_VIOLATIONS 14
#define PG_PROP_N_COUNTS 16
/* the limited quantities = the bits of `violated`: the weight in 1e-3, four counts, the sums of tables 0..3 in 1e-4 */
#define PG_PROP_L_WEIGHT 0
#define PG_PROP_L_HEAVY_ATOMS 1
#define PG_PROP_L_NHOH 2
#define PG_PROP_L_NO_COUNT 3
#define PG_PROP_L_ROTATABLE 4
#define PG_PROP_L_SUM0 5
#define PG_PROP_N_LIMITS 9
int pg_mol_props(const int8_t* cls, const int8_t* order, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                 const int* kekule_status /*[F][B]*/, const uint8_t* ring_size, const uint8_t* atom_ring, const int* g_lig_off /*[B+1]*/,
                 const int* g_bond_off /*[B+1]*/, int B, int F, int n_lig, int n_bond, int max_n, const int* tables /*device*/,
                 const int* table_rows /*[n_tables] host*/, int n_tables, const int* weights /*[PG_PROP_N_WEIGHTS] device*/,
                 const int* limits /*[PG_PROP_N_LIMITS][2] host*/, int max_violations, int* atom_env /*[F][n_lig]*/,
                 uint8_t* atom_row /*[F][PG_PROP_MAX_TABLES][n_lig]*/, int* sums /*[F][B][PG_PROP_MAX_TABLES]*/,
                 int* counts /*[F][B][PG_PROP_N_COUNTS]*/, int* weight_milli /*[F][B]*/, int* violated /*[F][B]*/, int* status /*[F][B]*/,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
