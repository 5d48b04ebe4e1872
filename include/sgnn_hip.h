/*
 * sgnn_hip.h — C ABI of libsgnn_hip.so, the MI355X (gfx950) sparse generative 3D
 * convolution hot path that sits behind SG-NN's `sparseconvnet` operator surface.
 *
 * Boundary being replaced.  The reference (angeladai/sgnn) reaches its sparse-op
 * arithmetic only through `import sparseconvnet as scn` (torch/model.py:7; call
 * sites torch/model.py:31-47, 178-188, 253-257, 296, 380).  Upstream's own native
 * boundary is a pybind11 module (`sparseconvnet.SCN`: class Metadata_3 plus
 * <Op>_updateOutput / <Op>_backward free functions taking at::Tensor&), i.e. not
 * a C ABI.  This header is the C ABI that takes its place; each entry point names
 * the scn operation / reference line it serves.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the comment says "host";
 *  - every function is asynchronous on `stream` (a hipStream_t passed as void*),
 *    performs no allocation and no device synchronisation;
 *  - the caller owns all memory (features, tables, hash storage, workspaces);
 *    workspace sizes come from the *_ws_bytes() queries;
 *  - return value: 0 = SGNN_OK, negative = error; sgnn_last_error() returns a
 *    thread-local message.  Nothing throws across the ABI;
 *  - coordinates are int32[4] = {z, y, x, batch} per site (16-byte rows), each
 *    spatial coordinate in [0, 65535], batch in [0, 32767]
 *    (layout contract: torch/scene_dataloader.py:13-36);
 *  - feature matrices are row-major float32 (N, C), contiguous.
 *  - neighbour / children tables are int32 [K][ld] (offset-major), -1 = no rule.
 *    A "rulebook" in upstream's sense is { (k, table[k][j], j) : table[k][j] >= 0 }.
 *  - capacity mode (device-side row counts): wherever a function takes a trailing `const int64_t *n_dev`
 *    (or nf_dev / m_dev ...), a non-NULL pointer makes the kernels read the row count from device memory at
 *    run time, clamped to the host value n, which then is only the CAPACITY the launch and the buffers are
 *    sized for.  The generative path (torch/model.py:229-247, 315-336) decides every level's row count from
 *    predicted logits; with the counts left on the device a whole training step has no host read-back and a
 *    fixed launch sequence, i.e. it can be captured in a HIP graph and replayed (sgnn_amd/train.py GraphStep).
 *    NULL = the host value is exact (the classic path).  Counts that exceed a capacity are clamped and
 *    SGNN_STATUS_OVERFLOW is raised in the status word; sgnn_adam_flat then leaves the parameters untouched.
 */
#ifndef SGNN_HIP_H
#define SGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGNN_OK 0
#define SGNN_EINVAL (-1)    /* bad argument */
#define SGNN_EHIP (-2)      /* HIP runtime / launch failure */
#define SGNN_EOVERFLOW (-3) /* size exceeds an internal 31-bit index */
#define SGNN_ENOWS (-4)     /* workspace too small */

/* status bits written (atomically OR-ed) into the device `status` word */
#define SGNN_STATUS_COORD_RANGE 1 /* a coordinate was outside the supported range ([0, 65535], batch [0, 32767]) — or, from
                                   * sgnn_rulebook_subm3_volume, outside the volume bounds the caller declared */
#define SGNN_STATUS_DUPLICATE 2   /* InputLayer(mode=0) saw the same site twice */
#define SGNN_STATUS_OVERFLOW 4    /* capacity mode: a level produced more rows than its buffers hold (step discarded) */

typedef void *sgnn_stream_t; /* hipStream_t */

const char *sgnn_last_error(void);
int sgnn_version(void);
/* name of the gfx target the kernels were compiled for ("gfx950") */
const char *sgnn_arch(void);

/* ---------------------------------------------------------------------------
 * Voxel hash grid — scn.InputLayer(3, size, mode=0) (torch/model.py:31,178,185,253)
 * ------------------------------------------------------------------------- */

/* capacity (power of two, >= 2n, >= 1024) of the open-addressing table for n sites */
int64_t sgnn_hash_capacity(int64_t n);

/* int64 [z,y,x,b] rows (the reference's LongTensor locs) -> int32 rows; sets
 * SGNN_STATUS_COORD_RANGE if a value is out of range */
int sgnn_coords_from_i64(const int64_t *locs, int64_t n, int32_t *coords, int32_t *status,
                         const int64_t *n_dev, sgnn_stream_t stream);
/* and back (metadata.getSpatialLocations, torch/model.py:380) */
int sgnn_coords_to_i64(const int32_t *coords, int64_t n, int64_t *locs, const int64_t *n_dev,
                       sgnn_stream_t stream);

/* build key->row table: keys[cap] (uint64), vals[cap] (int32).  The function
 * clears the table itself.  Sets SGNN_STATUS_DUPLICATE on repeated sites. */
int sgnn_hash_build(const int32_t *coords, int64_t n, uint64_t *keys, int32_t *vals, int64_t cap,
                    int32_t *status, const int64_t *n_dev, sgnn_stream_t stream);

/* row of each query site, or -1 (concat_skip join, torch/model.py:338-355) */
int sgnn_hash_lookup(const uint64_t *keys, const int32_t *vals, int64_t cap, const int32_t *query,
                     int64_t m, int32_t *rows, const int64_t *m_dev, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Measurement switches: ONE table.  Every kernel variant / launch fusion that was ever A/B-measured is selected by a field of
 * this struct; defaults are the measured winners.  No field changes results beyond fp32 / fp64 summation order (each entry
 * says what stays bit-identical).  No reference counterpart.  Set by name: sgnn_tune_set("conv_wide_epi", 0) returns the
 * previous value, SGNN_TUNE_UNKNOWN (with sgnn_last_error) for an unknown name or a value out of range; sgnn_tune_get reads;
 * sgnn_tune_names = the comma-separated field names; sgnn_tune_current = the live table (read-only).  Process-global, not
 * thread-safe: set them before the work they steer (workspace sizes follow conv_small_rows / conv_dw_blocks).
 * Host layer: sgnn_amd._lib.tune(name, value); environment SGNN_TUNE="name=value,name=value" at load.
 * ------------------------------------------------------------------------- */
#define SGNN_TUNE_UNKNOWN INT64_MIN
typedef struct sgnn_tune {
  /* levels below conv_small_rows run a latency-oriented kernel (16 rows per workgroup, the four waves split the offsets);
   * 0 = the 64-row variant of the big kernel.  The two sum the offsets in different orders (fp32 round-off).  Default 1. */
  int64_t conv_small;
  /* row count below which the small-level kernel is used.  Default 40 960. */
  int64_t conv_small_rows;
  /* levels above that run the wide-row 27-offset layers and every 8-offset walk as straight-line code (conv_unrolled.hip:
   * exact s_waitcnt counts, rule entries loaded up front); 0 = the looped kernel everywhere.  Bit-identical.  Default 1. */
  int64_t conv_unrolled;
  /* large levels: every workgroup of the rulebook walk takes as many consecutive 256-row tiles as it needs for ALL live
   * workgroups to be resident at once (no partial second round); 0 = one tile per workgroup.  Rows bit-identical; BatchNorm
   * statistics partials are summed per workgroup, so their fp64 grouping differs.  The tile count follows the workgroups of
   * the kernel the DEVICE holds at once (occupancy x compute units, queried per device on first use): statistics are
   * bit-reproducible for a given device model, driver and compiler, not across them — nor across library versions that
   * change a kernel's occupancy (the wide-row 26 / 30-channel straight-line kernels hold two workgroups per CU since their
   * weights stay resident in LDS, one before: their tile count per workgroup halved, their partials group differently).
   * Default 1. */
  int64_t conv_one_round;
  /* epilogue of the 256-row walk for output rows of 8 / 12 / 16 channels (torch/model.py:38-42, 180, 255, forward and data
   * gradient): 1 = the tile leaves the MFMA layout through a quad transpose, so the residual addend, the BatchNorm input of
   * the backward statistics and the output rows move as row-contiguous 16-byte accesses; 0 = one 4-byte access per
   * accumulator element.  Used when every row stride is a multiple of 4 floats and the bases are 16-byte aligned.  Stored
   * rows AND statistics partials bit-identical.  Default 1. */
  int64_t conv_wide_epi;
  /* row blocks a weight-gradient launch aims for (1 .. 4096; the launch is row blocks x offset groups workgroups).  Same
   * per-block sums in the same order for a given setting; the blocks' partial sums are added in block order.  Default 256. */
  int64_t conv_dw_blocks;
  /* weight gradient of a one-channel input (1 -> 8, the network's first convolution): 1 = the register-accumulating VALU
   * kernel, 0 = the MFMA kernel of the other shapes.  Different summation order (fp32 round-off).  Default 1. */
  int64_t conv_dw_c1;
  /* sgnn_rulebook_subm3_multi: 1 = all levels in one pre-fill launch and one builder launch, 0 = one sgnn_rulebook_subm3
   * per level.  Identical tables.  Default 1. */
  int64_t rulebook_multi;
  /* compactions / stride-2 levels: 1 = the write kernels sum the (<= 4096) raw block counts themselves, 0 = a scan launch
   * between the count and the write kernel.  Identical results.  Default 1. */
  int64_t scan_inline;
  /* sgnn_down2_chain_tables: 1 = the tables pass of level l and the hash insertion of level l + 1 in one launch.
   * Identical results.  Default 1. */
  int64_t chain_merged;
  /* sgnn_prog_forward / _backward: 0 switches the epilogue fusions off (conv -> AddTable, conv -> BatchNorm statistics,
   * in-place JoinTable): the per-layer launch sequence, identical arithmetic.  Default 1. */
  int64_t prog_fusion;
  /* a per-site linear head that is the only reader of a BatchNormReLU (the surface head): 1 = its data gradient dy w is
   * formed inside the two BatchNorm backward passes instead of being written and read back (bit-identical values); 0 =
   * k_linear_bwd writes it.  Applies to programs planned after the change.  Default 1. */
  int64_t prog_lin_bn;
  /* a per-site linear head whose input rows already carry a gradient when its backward pass runs (a Refinement's two heads,
   * torch/model.py:230-243): 1 = the head's kernel writes dy w + that gradient in one pass; 0 = an add launch over the level
   * follows.  Same sums (one fp32 addition per element either way).  Default 1. */
  int64_t prog_lin_add;
  /* BatchNorm forward / backward (bn.hip): 1 = small levels (c <= 64, few statistics partials) finalise the statistics
   * inside the apply kernels, as bn_fuse_ok decides; 0 = always the separate finalize kernels.  The two add the fp64
   * partials in different fixed orders (fp64 round-off before the fp32 results).  Default 1. */
  int64_t bn_fuse;
  /* sgnn_prog_forward / _backward (with prog_fusion and bn_fuse): a training-layout BatchNormReLU whose only reader is the
   * next op, a <= 16-channel convolution on a small level (the 16-row forward kernel and the one-offset weight gradient run there) and whose
   * statistics partials come from a convolution epilogue is not run as a pass of its own: the convolution sums the partial
   * table itself (in the order of the apply kernel), applies the layer to the rows it gathers, and its first workgroup stores
   * save_mean / save_invstd and updates the running statistics; the weight gradient applies the layer the same way.  The
   * layer's output buffer is never written (it keeps its slot: the gradient arena shares the layout and holds the layer's dy
   * there).  Outputs, statistics and gradients bit-identical.  0 = the layer runs as a pass.  Default 1. */
  int64_t prog_bn_fold_small;
} sgnn_tune;
int64_t sgnn_tune_set(const char *name, int64_t value);
int64_t sgnn_tune_get(const char *name);
const char *sgnn_tune_names(void);
const sgnn_tune *sgnn_tune_current(void);

/* ---------------------------------------------------------------------------
 * Rulebooks
 * ------------------------------------------------------------------------- */

/* 3x3x3 submanifold rulebook (scn.SubmanifoldConvolution, torch/model.py:32,38,40,179,186,254):
 * nbr[k*ld + j] = row of the site at p_j + d_k, k = (dz+1)*9+(dy+1)*3+(dx+1), else -1.
 * ld >= n.  With m = the live row count (n, or *n_dev clamped to n), the entries j in [m, min(roundup256(m), ld)) are
 * written as -1: the padding of the last 256-row tile that holds a live row, which is all the convolutions read.
 * Entries at or beyond roundup256(m) are unspecified (some paths write -1 there, none has to). */
int sgnn_rulebook_subm3(const uint64_t *keys, const int32_t *vals, int64_t cap,
                        const int32_t *coords, int64_t n, int32_t *nbr, int64_t ld,
                        const int64_t *n_dev, sgnn_stream_t stream);

/* `count` <= SGNN_RULEBOOK_MULTI_MAX such rulebooks in one pair of launches (capacity mode: every n_devs[i] != NULL):
 * the coarse levels of one hierarchy (scn.InputLayer + the Convolution(2,2) chain, torch/model.py:228-236) have
 * 0.4 k - 40 k rows each and their single launches are mostly ramp.  Each array holds one entry per level with the
 * meaning of the matching sgnn_rulebook_subm3 argument; table i equals sgnn_rulebook_subm3's for level i entry by
 * entry.  Levels with ns[i] == 0 are skipped. */
#define SGNN_RULEBOOK_MULTI_MAX 4
int sgnn_rulebook_subm3_multi(int count, const uint64_t *const *keys, const int32_t *const *vals, const int64_t *caps,
                              const int32_t *const *coords, const int64_t *ns, int32_t *const *nbrs, const int64_t *lds,
                              const int64_t *const *n_devs, sgnn_stream_t stream);

/* The same table through a dense index volume (volume[((b*Z + z)*Y + y)*X + x] = row, -1 elsewhere): one coalesced
 * 4-byte read per neighbour instead of a hash probe.  `volume` is a persistent workspace of volume_entries int32 that
 * the caller fills with -1 ONCE; the call marks this level's rows, builds the table and clears the rows again, so the
 * volume is all -1 on return.  Blocks with batch index >= volume_entries / (Z*Y*X) and positions outside [0, dims) go
 * through the hash grid (keys / vals / cap): the table equals sgnn_rulebook_subm3's for every input.
 * One volume serves one stream at a time (calls are stream-ordered by the caller).  Measured at N = 366 k (64^3 x 32
 * blocks): 18 us against 97 us for sgnn_rulebook_subm3 (profiles/r02j_rulebook.txt). */
int sgnn_rulebook_subm3_dense(const uint64_t *keys, const int32_t *vals, int64_t cap, const int32_t *coords, int64_t n,
                              int dim_z, int dim_y, int dim_x, int32_t *volume, int64_t volume_entries, int32_t *nbr,
                              int64_t ld, const int64_t *n_dev, sgnn_stream_t stream);
/* The same table for a level whose sites are known to lie inside the volume (the generated levels: children of a dense
 * coarse volume bounded by the model's own sizes, torch/model.py:192-207): volume only, no hash grid of the level is read —
 * or built.  A site the volume does not cover raises SGNN_STATUS_COORD_RANGE in *status. */
int sgnn_rulebook_subm3_volume(const int32_t *coords, int64_t n, int dim_z, int dim_y, int dim_x, int32_t *volume,
                               int64_t volume_entries, int32_t *nbr, int64_t ld, const int64_t *n_dev, int32_t *status,
                               sgnn_stream_t stream);

/* stride-2 / size-2 rulebook, phase 1 (scn.Convolution(...,2,2), torch/model.py:44):
 * finds the coarse active set unique(floor(p/2)) in FIRST-TOUCH order of the fine
 * rows (wave ballot + prefix-sum compaction), writes
 *   parent[i]              coarse row of fine site i
 *   coarse_coords[c*4..]   coordinates of coarse row c   (room for nf rows)
 *   ckeys/cvals (ccap)     hash grid of the coarse level (key -> coarse row)
 *   *n_coarse (device)     number of coarse sites
 * ccap = sgnn_hash_capacity(nf).  Values of empty hash slots are unspecified; nf = 0 leaves an empty hash and count 0.
 * This is sgnn_down2_chain at depth 1 with the row count on the host: 5 launches (6 with sgnn_tune.scan_inline = 0).
 * Workspace (sgnn_down2_ws_bytes): slot and rank of every fine row, the owner table (ccap ints), the block sums.  The
 * three *_ws_bytes queries of this section presume ccap = sgnn_hash_capacity(rows); a call with a larger ccap needs
 * 4 * (ccap - sgnn_hash_capacity(rows)) more bytes per level slice and is refused (SGNN_ENOWS) without them. */
int64_t sgnn_down2_ws_bytes(int64_t nf);
int sgnn_rulebook_down2(const int32_t *fine_coords, int64_t nf, uint64_t *ckeys, int32_t *cvals,
                        int64_t ccap, int32_t *parent, int32_t *coarse_coords, int64_t *n_coarse,
                        void *ws, int64_t ws_bytes, sgnn_stream_t stream);
/* phase 2, once the host knows n_coarse: offset-major tables
 *   children[k*ldc + c] = fine row whose parent is c and whose offset
 *                         (z&1)*4+(y&1)*2+(x&1) is k, else -1        (8 x ldc)
 *   ptable[k*ldf + i]   = parent[i] if offset(i)==k else -1          (8 x ldf)
 * (padding entries are written as -1 up to min(roundup256(live coarse rows), ldc) / min(roundup256(live fine rows), ldf);
 *  entries beyond are unspecified, as for sgnn_rulebook_subm3)
 * children drives the forward conv / unpool-backward, ptable the data-gradient. */
int sgnn_down2_tables(const int32_t *fine_coords, const int32_t *parent, int64_t nf,
                      int32_t *children, int64_t ldc, int64_t nc, int32_t *ptable, int64_t ldf,
                      const int64_t *nf_dev, const int64_t *nc_dev, sgnn_stream_t stream);

/* Phase 1 for `depth` successive levels in one submission (a U-Net's whole stride-2 pyramid), row counts staying on
 * the device: level 0 = fine_coords with *n0_dev rows (n0_dev NULL: n0 rows), at most `cap` rows; for l < depth it
 * writes parent[l] (cap ints: coarse row of every site of level l), coarse_coords[l] (cap x 4), the hash of level l+1
 * (ckeys[l], cvals[l]; ccap = sgnn_hash_capacity(cap) each) and counts_dev[l] = rows of level l+1.  ckeys .. coarse_coords
 * are HOST arrays of device pointers.  Results are identical to `depth` calls of sgnn_rulebook_down2 (first-touch
 * order); the host reads all counts with one copy and then calls sgnn_down2_tables per level.
 * Capacity mode: level_caps (HOST array, depth entries, or NULL) clamps counts_dev[l] to the capacity of the buffers
 * that will hold level l+1's features and raises SGNN_STATUS_OVERFLOW in *status when it had to.
 * 5 launches per level (init, insert, count, write, parent), 6 with sgnn_tune.scan_inline = 0 (the scan of the block
 * counts).  Workspace (sgnn_down2_chain_ws_bytes): the scratch of one level (slot and rank of `cap` rows, owner table
 * of ccap ints, block sums), used by every level in turn. */
int64_t sgnn_down2_chain_ws_bytes(int64_t cap);
int sgnn_down2_chain(const int32_t *fine_coords, int64_t n0, const int64_t *n0_dev, int64_t cap, int depth,
                     void *const *ckeys, void *const *cvals, int64_t ccap, void *const *parent,
                     void *const *coarse_coords, int64_t *counts_dev, const int64_t *level_caps, int32_t *status,
                     void *ws, int64_t ws_bytes, sgnn_stream_t stream);

/* Capacity mode: the pyramid AND its tables in one submission — sgnn_down2_chain (row counts from *n0_dev, clamped to
 * level_caps, SGNN_STATUS_OVERFLOW) followed by sgnn_down2_tables of every level, as 3 launches per level + 2 (one init
 * for all levels, the insertion of level 0; per level count, write kernel, parent + tables pass, which also runs the next
 * level's insertion; 5 per level + 1 with sgnn_tune.scan_inline = 0 / chain_merged = 0) instead of 8 per level.
 * children[l] is (8 x ldc_l), ldc_l = roundup256(min(level_caps[l], cap)); ptable[l] is (8 x ldf_l),
 * ldf_0 = roundup256(cap), ldf_l = ldc_{l-1}.  Only rows below roundup256(live count) of a table are written (and read).
 * Workspace (sgnn_down2_chain_tables_ws_bytes): sgnn_down2_chain's level scratch once per level, one set of block sums. */
int64_t sgnn_down2_chain_tables_ws_bytes(int64_t cap, int depth);
int sgnn_down2_chain_tables(const int32_t *fine_coords, const int64_t *n0_dev, int64_t cap, int depth,
                            void *const *ckeys, void *const *cvals, int64_t ccap, void *const *parent,
                            void *const *coarse_coords, int64_t *counts_dev, const int64_t *level_caps,
                            void *const *children, void *const *ptable, int32_t *status, void *ws, int64_t ws_bytes,
                            sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sparse convolution: out[j] = sum_k W[k]^T x[table[k][j]]   (fp32 MFMA 16x16x4)
 * serves SubmanifoldConvolution fwd (table = nbr, K = 27), Convolution(2,2) fwd
 * (table = children, K = 8) and both data-gradients:
 *   subm  dX: x := dY, table = nbr,    flags = TRANSPOSE_W | FLIP_K
 *   down2 dX: x := dY, table = ptable, flags = TRANSPOSE_W
 * w is always the layer's weight (K, c_in_layer, c_out_layer); with TRANSPOSE_W the
 * call's cin/cout are (c_out_layer, c_in_layer).
 * in_shift: feature row = table value >> in_shift (3 = features live on the
 * parents of an 8-child expansion, torch/model.py:192-207; 0 otherwise).
 * n_in = rows of x.  Table layout contract for the conv entry points: ld is a multiple of 256
 * and the padding entries table[k][m .. roundup256(m)) are -1, m = the live output rows (n_out, or the device count
 * clamped to it): a table is read in tiles of at most 256 rows that start below m (every table this library builds is so);
 * K <= 64; each slab (x, y, table) must be smaller than 4 GiB (raw-buffer addressing).
 * ------------------------------------------------------------------------- */
#define SGNN_CONV_TRANSPOSE_W 1
#define SGNN_CONV_FLIP_K 2
int sgnn_conv_fwd(const float *x, int64_t n_in, int cin, const float *w, int K, const int32_t *table,
                  int64_t ld, int64_t n_out, int cout, float *y, int flags, int in_shift,
                  sgnn_stream_t stream);

/* Generalised rulebook walk (used for the generative up-sampling convolution, see below):
 *   offset k of group g reads table row kmap[g*K + k]       (kmap NULL: row k)
 *   and gathers feature row  (entry >> in_shift)*in_mul + kadd[g*K + k]   (kadd NULL: + 0)
 *   group g uses the weight block w + g*K*cin*cout and owns output rows  row*groups + g
 * so y has n_out*groups rows.  kmap and kadd (groups*K ints each) are device arrays; table_rows =
 * number of offset rows the table really has (27 for a 3x3x3 rulebook).
 * Generative up-sampling (Refinement.n0/n1, torch/model.py:185-186,220-223): all 8 children of a site
 * carry its features (model.py:203), so SubmanifoldConvolution on the 8N children collapses, per child
 * parity g, into 8 parent-level offsets with pre-summed weights: forward = one launch with groups = 8,
 * K = 8 on the PARENT table (3.4x fewer gathers and flops than 27 offsets on 8N rows; the children
 * grid and its rulebook are never built); data gradient = K = 64 offsets with in_mul = 8, kadd = parity, run as 4 groups of 16 offsets whose
 * partial rows are added by sgnn_sum_groups (more workgroups, shorter offset walk per workgroup). */
int sgnn_conv_fwd_ex(const float *x, int64_t n_in, int cin, const float *w, int K, const int32_t *table,
                     int64_t ld, int64_t n_out, int cout, float *y, int flags, int in_shift,
                     const int32_t *kmap, const int32_t *kadd, int in_mul, int groups, int table_rows,
                     sgnn_stream_t stream);
int sgnn_conv_bwd_weight_ex(const float *x, int64_t n_in, int cin, const float *dy, int cout,
                            const int32_t *table, int64_t ld, int K, int64_t n_out, float *dw, int in_shift,
                            const int32_t *kmap, const int32_t *kadd, int in_mul, int groups, int table_rows,
                            void *ws, int64_t ws_bytes, sgnn_stream_t stream);

/* Plain rulebook walk with strided rows and a fused epilogue (what the program executor uses to remove the
 * AddTable / BatchNorm-statistics passes around a convolution, torch/model.py:33-42 and the FullyConvolutionalNet
 * blocks):
 *   x rows have stride ldx floats, y rows ldy, addend rows ld_add (0 = contiguous);
 *   y = conv + addend when addend != NULL (addend may be y itself: accumulate in place);
 *   stats = 1: partial[blk][0][c] = sum over the workgroup's rows of y, [1][c] = sum of y*y;
 *   stats = 2: y is the gradient w.r.t. a BatchNormReLU output whose INPUT rows are bn_x (stride ld_bnx) with
 *              mean / invstd / gamma / beta (gamma, beta may be NULL) and leak: partial = sum dz, sum dz*xhat with
 *              dz = y * (bn_out > 0 ? 1 : leak) — the reduction BatchNorm backward starts with.
 * partial holds sgnn_conv_stats_blocks(n_out) * 2 * cout doubles; sgnn_bn_fwd_ex / sgnn_bn_bwd_ex accept it as
 * pre_partial.  Only for the compiled (cin, cout) shapes; SGNN_EINVAL otherwise. */
int64_t sgnn_conv_stats_blocks(int64_t n_out);
int sgnn_conv_fwd_epi(const float *x, int64_t n_in, int cin, int64_t ldx, const float *w, int K,
                      const int32_t *table, int64_t ld, int64_t n_out, int cout, float *y, int64_t ldy, int flags,
                      const float *addend, int64_t ld_add, int stats, double *partial, const float *bn_x,
                      int64_t ld_bnx, const float *mean, const float *invstd, const float *gamma, const float *beta,
                      float leak, sgnn_stream_t stream);

/* weight gradient dW[k][ci][co] = sum_j x[table[k][j]][ci] * dy[j][co]; deterministic
 * two-stage reduction through the workspace. */
int64_t sgnn_conv_bwd_weight_ws_bytes(int64_t n_out, int K, int cin, int cout);
int sgnn_conv_bwd_weight(const float *x, int64_t n_in, int cin, const float *dy, int cout,
                         const int32_t *table, int64_t ld, int K, int64_t n_out, float *dw, int in_shift, void *ws,
                         int64_t ws_bytes, sgnn_stream_t stream);

/* pre-summed weights of the generative up-sampling convolution and their gradient: Wc (64, cin, cout) from the layer's
 * W (27, cin, cout); dW from dWc (see sgnn_conv_fwd_ex) */
int sgnn_expand_weights(const float *w, int cin, int cout, float *wc, sgnn_stream_t stream);
int sgnn_expand_weights_bwd(const float *dwc, int cin, int cout, float *dw, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * scn.BatchNormReLU / BatchNormalization (torch/model.py:37,39,42,45,181,187,256)
 * leak: 0 = ReLU, 1 = plain batch norm.  momentum = fraction of OLD running value kept.
 * training: batch statistics (biased var to normalise, unbiased into running_var),
 * save_mean/save_invstd (C floats each) kept for backward.
 * ------------------------------------------------------------------------- */
int64_t sgnn_bn_ws_bytes(int64_t n, int c);
int sgnn_bn_fwd(const float *x, int64_t n, int c, const float *gamma, const float *beta,
                float *running_mean, float *running_var, float eps, float momentum, int training,
                float leak, float *save_mean, float *save_invstd, float *y, void *ws,
                int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_bn_bwd(const float *x, const float *dy, int64_t n, int c, const float *gamma,
                const float *beta, const float *save_mean, const float *save_invstd, int training,
                float leak, float *dx, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes,
                sgnn_stream_t stream);
/* same, with dx = (BatchNorm gradient) + addend[...]; addend may be dx itself (in-place accumulation) or NULL */
int sgnn_bn_bwd_add(const float *x, const float *dy, int64_t n, int c, const float *gamma, const float *beta,
                    const float *save_mean, const float *save_invstd, int training, float leak,
                    const float *addend, float *dx, float *dgamma, float *dbeta, void *ws, int64_t ws_bytes,
                    sgnn_stream_t stream);

/* strided rows (ldx, ldy, ... in floats; 0 = c) and optional statistics partials from a convolution epilogue
 * (pre_partial / pre_nblk, see sgnn_conv_fwd_epi): the statistics pass is skipped */
int sgnn_bn_fwd_ex(const float *x, int64_t ldx, int64_t n, int c, const float *gamma, const float *beta,
                   float *running_mean, float *running_var, float eps, float momentum, int training, float leak,
                   float *save_mean, float *save_invstd, float *y, int64_t ldy, const double *pre_partial,
                   int64_t pre_nblk, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_bn_bwd_ex(const float *x, int64_t ldx, const float *dy, int64_t ld_dy, int64_t n, int c, const float *gamma,
                   const float *beta, const float *save_mean, const float *save_invstd, int training, float leak,
                   const float *addend, int64_t ld_add, float *dx, int64_t ld_dx, float *dgamma, float *dbeta,
                   const double *pre_partial, int64_t pre_nblk, void *ws, int64_t ws_bytes, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Row movement (all pure copies / sums, fp32 rows of c floats).  Rows move as float4 when c % 4 == 0 and every base
 * pointer is 16-byte aligned, float by float otherwise (a contiguous view at an odd float offset of a larger buffer);
 * same values either way.
 * ------------------------------------------------------------------------- */
/* Up to 8 device-to-device copies as one launch: dst[k] <- src[k], bytes[k] bytes each (host arrays of device pointers /
 * sizes; regions must not overlap each other).  train.GraphStep loads a batch into the replayed graph's static input
 * buffers with it (torch/train.py:256-262 uploads the batch there): one kernel instead of seven copies per step. */
int sgnn_copy_multi(void *const *dst, const void *const *src, const int64_t *bytes, int nregions, sgnn_stream_t stream);

/* dst[r] = src[idx[r]]  (UnPooling fwd: idx = parent; mask compaction: idx = sel) */
int sgnn_gather_rows(const float *src, int c, const int32_t *idx, int64_t m, float *dst,
                     sgnn_stream_t stream);
/* the same with the row count read from device memory (*m_dev <= m_cap): no host round trip between a mask
 * compaction and the consumers of the compacted coordinates */
int sgnn_gather_rows_dn(const float *src, int c, const int32_t *idx, const int64_t *m_dev, int64_t m_cap,
                        float *dst, sgnn_stream_t stream);
/* dst[r] = [ a[ia?ia[r]:r] | b[ib?ib[r]:r] | c[ic?ic[r]:r] ]  (negative index -> zeros, zero-channel sources skipped) and
 * its gradient (indices unique; destinations reached through an index array are zero-filled first, NULL ones skipped) */
int sgnn_concat3_rows(const float *a, int ca, const int32_t *ia, const float *b, int cb, const int32_t *ib,
                      const float *c, int cc, const int32_t *ic, int64_t m, float *dst, sgnn_stream_t stream);
int sgnn_concat3_rows_bwd(const float *ddst, int ca, const int32_t *ia, int cb, const int32_t *ib, int cc,
                          const int32_t *ic, int64_t m, float *da, int64_t na, float *db, int64_t nb, float *dc,
                          int64_t nc, sgnn_stream_t stream);
/* dst (n_dst rows, zero-filled here) ; dst[idx[r]] = src[r]   (idx unique) */
int sgnn_scatter_rows(const float *src, int c, const int32_t *idx, int64_t m, float *dst,
                      int64_t n_dst, const int64_t *m_dev, sgnn_stream_t stream);
/* dst[j] = sum_k src[table[k*ld+j]] over valid entries (UnPooling bwd: table = children) */
int sgnn_gather_sum(const float *src, int c, const int32_t *table, int64_t ld, int K,
                    int64_t n_out, float *dst, sgnn_stream_t stream);
/* dst[r*rep + t] = src[r]  (to_next_level_locs feature replication, torch/model.py:203) */
int sgnn_repeat_rows(const float *src, int c, int64_t n, int rep, float *dst, sgnn_stream_t stream);
/* dst[r] = sum_t src[r*rep + t]  (its gradient) */
int sgnn_sum_groups(const float *src, int c, int64_t n, int rep, float *dst, sgnn_stream_t stream);
/* dst[r] = [ a[ia ? ia[r] : r] | (ib ? (ib[r] >= 0 ? b[ib[r]] : 0) : b[r]) ]
 * serves JoinTable (ia = ib = NULL), concat_skip (ib = hash_lookup rows, torch/model.py:354)
 * and the fused mask-compaction concat (ia = ib = sel, torch/model.py:242,330) */
int sgnn_concat_rows(const float *a, int ca, const int32_t *ia, const float *b, int cb,
                     const int32_t *ib, int64_t m, float *dst, sgnn_stream_t stream);
/* gradient of sgnn_concat_rows: da (na rows) / db (nb rows) are zero-filled here when the
 * matching index is given; indices are unique so no atomics are needed.  da or db may be NULL. */
int sgnn_concat_rows_bwd(const float *ddst, int ca, const int32_t *ia, int cb, const int32_t *ib,
                         int64_t m, float *da, int64_t na, float *db, int64_t nb,
                         sgnn_stream_t stream);
/* y = a + b  (scn.AddTable) */
int sgnn_add(const float *a, const float *b, int64_t count, float *y, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Generative glue
 * ------------------------------------------------------------------------- */
/* children coords: out[(8i+j)] = {2z+dz, 2y+dy, 2x+dx, b}, j = 4dz+2dy+dx
 * (Refinement.to_next_level_locs, torch/model.py:192-207) */
int sgnn_expand8_coords(const int32_t *coords, int64_t n, int32_t *out, const int64_t *n_dev, sgnn_stream_t stream);
/* the same, also writing the children as the int64 (z, y, x, b) rows the model returns per level (torch/model.py:207,243;
 * = sgnn_coords_to_i64 of `out`) in the same pass */
int sgnn_expand8_coords_i64(const int32_t *coords, int64_t n, int32_t *out, int64_t *locs, const int64_t *n_dev,
                            sgnn_stream_t stream);
/* all voxel coordinates of a dense (B, d0, d1, d2) volume, batch-major raster order
 * (GenModel.dense_coarse_to_sparse, torch/model.py:319-321) */
int sgnn_dense_coords(int batch, int d0, int d1, int d2, int32_t *out, sgnn_stream_t stream);
/* stable compaction: sel[0..count) = ascending rows i with sigmoid(logits[i*stride]) > 0.5
 * (torch/model.py:233,322); wave ballot + prefix sum.  *count is a device int64. */
int64_t sgnn_compact_ws_bytes(int64_t n);
int sgnn_compact_sigmoid(const float *logits, int64_t stride, int64_t n, int32_t *sel,
                         int64_t *count, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
/* same for an explicit uint8 mask */
/* teacher forcing: keep site i iff the dense (B,1,d0,d1,d2) float volume is > 0.5 at coords[i] = {z,y,x,b} */
int sgnn_compact_dense(const int32_t *coords, int64_t n, const float *vol, int batch, int d0, int d1, int d2,
                       int32_t *sel, int64_t *count, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_compact_mask(const uint8_t *mask, int64_t n, int32_t *sel, int64_t *count, void *ws,
                      int64_t ws_bytes, sgnn_stream_t stream);
/* capacity mode of the two generative mask compactions: the number of candidates is *n_dev (NULL: n), the kept count
 * count2[0] is clamped to keep_cap (SGNN_STATUS_OVERFLOW in *status otherwise) and count2[1] = 8 * count2[0], the row
 * count of the kept sites' 8-child expansion (torch/model.py:192-207), is published with it */
int sgnn_compact_sigmoid_cap(const float *logits, int64_t stride, int64_t n, const int64_t *n_dev, int32_t *sel,
                             int64_t *count2, int64_t keep_cap, int32_t *status, void *ws, int64_t ws_bytes,
                             sgnn_stream_t stream);
int sgnn_compact_dense_cap(const int32_t *coords, int64_t n, const int64_t *n_dev, const float *vol, int batch, int d0,
                           int d1, int d2, int32_t *sel, int64_t *count2, int64_t keep_cap, int32_t *status, void *ws,
                           int64_t ws_bytes, sgnn_stream_t stream);
/* the same two, also writing locs[r] = coords[sel[r]] (16-byte {z,y,x,b} rows) for the kept rows r < keep_cap: the next
 * level's site list (torch/model.py:236-243) without a gather launch of its own */
int sgnn_compact_sigmoid_cap_locs(const float *logits, int64_t stride, int64_t n, const int64_t *n_dev,
                                  const int32_t *coords, int32_t *sel, int32_t *locs, int64_t *count2, int64_t keep_cap,
                                  int32_t *status, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_compact_dense_cap_locs(const int32_t *coords, int64_t n, const int64_t *n_dev, const float *vol, int batch, int d0,
                                int d1, int d2, int32_t *sel, int32_t *locs, int64_t *count2, int64_t keep_cap,
                                int32_t *status, void *ws, int64_t ws_bytes, sgnn_stream_t stream);

/* scn.SparseToDense (torch/model.py:47): dense (B, C, d0, d1, d2) zero-filled here */
int sgnn_sparse_to_dense(const float *feats, const int32_t *coords, int64_t n, int c, float *dense,
                         int batch, int d0, int d1, int d2, sgnn_stream_t stream);
/* feats[r][ch] = dense[b][ch][z][y][x] at coords[r]  (its gradient, and the NCDHW -> rows
 * permute of dense_coarse_to_sparse, torch/model.py:324-327) */
int sgnn_dense_to_sparse(const float *dense, const int32_t *coords, int64_t n, int c, float *feats,
                         int batch, int d0, int d1, int d2, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Per-site linear heads y[r] = W x[r] + b, W (cout, cin) row-major, cout <= 2
 * (nn.Linear(nf,1) x2 fused, torch/model.py:190-191,230-231; SurfacePrediction.linear :258,271).
 * bwd: dx (may be NULL), dw (cout, cin), dbias (may be NULL); deterministic reduction via ws.
 * ------------------------------------------------------------------------- */
int64_t sgnn_linear_ws_bytes(int64_t n, int cin, int cout);
int sgnn_linear_fwd(const float *x, int64_t n, int cin, const float *w, const float *bias, int cout,
                    float *y, sgnn_stream_t stream);
int sgnn_linear_bwd(const float *x, const float *dy, int64_t n, int cin, const float *w, int cout,
                    float *dx, float *dw, float *dbias, void *ws, int64_t ws_bytes,
                    sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused hierarchical loss, all levels (n <= 5; a single level is n = 1) in two launches
 * forward and one backward.  Per level: sparse predictions vals (m, vstride) at locs (m,4) int64 [z,y,x,b] against
 * dense (B,1,d0,d1,d2) targets —
 *   out2s[2l]   = mean over kept sites of w * BCE_with_logits(vals[:,occ_col], tgt_occ)   (torch/loss.py:58-82)
 *   out2s[2l+1] = mean over kept sites of w * |logt(vals[:,sdf_col]) - logt(tgt_sdf)|      (torch/loss.py:122-157)
 * occ_col / sdf_col = -1 skips that term; weights / known may be NULL.
 * mask_mode 0: keep every site (UNK_ID occupancy targets count as 0); 1: keep tgt_occ != -1; 2: keep known < 2.
 * m_dev (device int64, may be NULL): the live row count in capacity mode; a level whose count is <= 0 contributes 0.
 * sums (3n doubles, device) carries {sum bce, sum l1, kept} of every level to the backward call.
 *   total  = sum_i coef[i] * out2s[i] over the slots with coef[i] != 0                     (torch/loss.py:160-199)
 *   cur[l] = out2s[2l] + out2s[2l+1] restricted to those slots (the per-level values for logging)
 *   dvals_l[:, occ_col] = g * coef[2l] * d bce_l,  dvals_l[:, sdf_col] = g * coef[2l+1] * d l1_l, other columns 0
 * levels: HOST array of n x 16 int64 = {locs, vals, vstride, occ_col, sdf_col, tgt_occ, tgt_sdf, weights, known, d0, d1,
 * d2, m, use_log, mask_mode, m_dev} (device pointers as integers); coef_host: 2n floats = (bce, l1) weight per level;
 * out2s (2n floats), total, cur (n floats): device; g: device float = d loss / d total; dvals: HOST array of n device
 * pointers, (m_l, vstride_l) floats each.  The fp64 two-stage reduction has a fixed order per level, which depends on
 * that level's m alone: the same level gives the same bits whichever other levels share the call.
 * Contracts: every row of locs, rows past the live count included, must lie inside its (B, d0, d1, d2) volume (the
 * kernels gather without a bounds check) and locs must be 16-byte aligned (it is read with 16-byte loads); dvals rows
 * past the live count min(max(*m_dev, 0), m) are left unwritten, rows below it are written in every column (+0 for a
 * row that is not kept and for the columns other than occ_col / sdf_col).
 * ------------------------------------------------------------------------- */
int64_t sgnn_loss_multi_ws_bytes(void);
int sgnn_loss_levels_fwd(const int64_t *levels, int n, const float *coef_host, double *sums, float *out2s, float *total,
                         float *cur, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_loss_levels_bwd(const int64_t *levels, int n, const float *coef_host, const double *sums, const float *g,
                         void *const *dvals, sgnn_stream_t stream);

/* Targets of the hierarchical loss in three launches — compute_targets + compute_weights_missing_geo
 * (torch/loss.py:15-32, 35-48): tsdf = clamp(sdf, +-trunc); hier_last = tsdf; occ_last = |tsdf| < trunc with UNK_ID (-1)
 * where known >= 2 (masking); w_last = weight_missing_geo off the input sites, 1 on them; and for the ncoarse (<= 3)
 * coarser levels, listed from the second finest downwards in the host pointer arrays hier_in / occ / w / hier:
 * occ = 2x2x2 max-pool of the level above, w = that level's w[::2,::2,::2], hier = clamp(hier_in).  w_last NULL: no
 * weights.  input_locs = the (n_locs, 4) int64 [z,y,x,b] input sites, of which the first min(max(*n_locs_dev, 0), n_locs)
 * count (n_locs_dev NULL: all); a site outside the (batch, d0, d1, d2) volume is skipped.  The clamp keeps NaN, like
 * torch.clamp_.  Dimensions must be divisible by 2^ncoarse; every output must be 8-byte aligned. */
int sgnn_loss_targets(const float *sdf, const uint8_t *known, const int64_t *input_locs, int64_t n_locs,
                      const int64_t *n_locs_dev, int batch,
                      int d0, int d1, int d2, float trunc, int masking, float weight_missing_geo, int ncoarse,
                      void *const *hier_in, float *tsdf, float *hier_last, float *occ_last, float *w_last,
                      void *const *occ, void *const *w, void *const *hier, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sparse-network programs: a static sub-network (what the reference composes from scn.Sequential /
 * ConcatTable / AddTable / JoinTable containers, torch/model.py:31-47, 178-188, 253-257) compiled into a
 * flat op list and run forward / backward from ONE call — same kernels, same order, bit-identical to the
 * per-layer entry points, no host round trip per layer.  All descriptor arrays are HOST memory:
 *   ops   int32[nops][8] = {type, in0, in1, out, param, level, cin, cout}
 *         type 0 subm conv, 1 stride-2 conv (level -> level+1), 2 unpool (out on `level`, in0 on level+1),
 *         3 batch-norm (param .. param+3 = gamma, beta, running_mean, running_var), 4 add, 5 join
 *         (cin / cout = channels of in0 / in1)
 *   opf   float[nops][4] = {eps, momentum, leak, 0}
 *   bufs  int32[nbuf][2] = {level, channels}; buffer 0 is the input
 *   ops are 12 ints each: type, in0, in1, out, param slot, level, cin, cout, in2, ia, ib, ic.  Types 0..5 are the scn
 *         containers' leaves (SUBM conv, stride-2 conv, UnPooling, BatchNorm(ReLU), AddTable, JoinTable); 6 =
 *         CONCAT_IN out = [in0[ia] | in1[ib] | in2[ic]] (the skip join + feature hand-over between generative
 *         stages, torch/model.py:242, 330, 338-355; ia/ib/ic index the idx[] array of int32 device arrays, -1 = rows
 *         as they are); 7 = the 8-child up-sampling convolution on the parent rulebook (out has 8x the rows); 8 =
 *         linear heads (weight row o = slot par+2o, bias par+2o+1).  Buffers [0, n_ext) are caller-owned inputs
 *         (ext[] pointers; their gradients go to gext[]), the rest live in the arena.
 *   lev_* per level: rows, table ld, nbr table, and for the transition level -> level+1 the children /
 *         ptable tables and the parent array (device pointers, NULL where unused); a JoinTable's inputs are column ranges of its output (no concat pass) unless `keep`
 *         asks for one of them; lev_cnt (the array may be NULL): per rows class a device int64 with the live row
 *         count (capacity mode, see the conventions above; lev_n then holds the capacities) or NULL
 *   params / pgrads: host arrays of device pointers.
 * Feature buffers live in a caller-owned arena (sgnn_prog_arena_floats floats; layout via
 * sgnn_prog_buffer_offset); `input` optionally points buffer 0 outside the arena.  Backward: garena has the
 * same layout, the caller fills the output gradients and flags them in ginit[nbuf].
 * keep[nbuf] (host, may be NULL) flags the buffers the caller reads after the forward call (outputs / taps): the
 * executor fuses conv -> AddTable and conv -> BatchNorm statistics into the convolution epilogue and then never
 * materialises the convolution's own output buffer unless it is flagged; a JoinTable whose inputs can be produced in
 * place gets no copy (its inputs live in column ranges of the join buffer and are read / written through a row
 * stride).  The same `keep` must be passed to the arena / offset queries and to the backward call (the layout depends
 * on it).  sgnn_tune.prog_fusion = 0 switches the fusions off (A/B measurements, parity tests).
 * ------------------------------------------------------------------------- */
/* mode 0: floats of the gradient arena sgnn_prog_backward needs (buffers + per-op areas + backward scratch);
 * mode 1: floats of the arena sgnn_prog_forward needs (buffers + per-op areas);
 * mode 2: the same for an INFERENCE call (sgnn_prog_forward with training = 2): no backward pass may follow, so a
 *         buffer's storage is reused once its last reader has run — the arena is the high-water mark of the live set,
 *         3-4x smaller for a U-Net stage (whole-scene inference, BASELINE configs[3]);
 * mode 3: the same with bf16 storage (sgnn_prog_forward with training = 2 | 4).  Still counted in floats: a buffer of
 *         n rows takes ceil(n * ld / 2) floats, ld = its channels rounded up to a multiple of 8 bf16 elements; LINEAR
 *         outputs stay fp32 (ld = channels).  sgnn_prog_buffer_offset: infer = 2 gives this layout's offsets
 *         (for an external: the offset of its bf16 copy, -1 if it has none). */
int64_t sgnn_prog_arena_floats(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext,
                               const int64_t *lev_n, int nlev, const int32_t *keep, int mode);
int64_t sgnn_prog_ws_bytes(const int32_t *ops, int nops, const int64_t *lev_n, int nlev);
int64_t sgnn_prog_buffer_offset(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext,
                                const int64_t *lev_n, int nlev, const int32_t *keep, int infer, int b);
/* What the executor decides for these descriptors under the current sgnn_tune switches (tests, diagnostics): host only,
 * launches nothing, takes no stream.  mode as in sgnn_prog_arena_floats (3: the plan of the bf16 layout).
 * out int32[4 * nops + 3 * nbuf]: per op {skip (the forward pass launches nothing for it), add_dst (>= 0: the
 * convolution stores the sum of the AddTable behind it into that buffer), join_view (the JoinTable is in place),
 * lin_bn (>= 0: the head's data gradient is formed inside the backward pass of that BatchNorm op)}, then per buffer
 * {root (the buffer whose storage it lives in), col (its column offset there), ld (its row stride in elements)}. */
int sgnn_prog_plan(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext, const int64_t *lev_n,
                   int nlev, const int32_t *keep, int mode, int32_t *out);
/* training: 0 = eval, 1 = training (batch statistics), | 2 = inference layout (see sgnn_prog_arena_floats mode 2),
 * | 4 = bf16 storage (mode 3; only as 2 | 4, eval: running statistics).  In the bf16 layout the externals stay fp32,
 * every arena buffer is bf16 except the LINEAR outputs (fp32 logits); math is fp32 with one rounding per stored value.
 * wait_event (hipEvent_t or NULL): the stream waits for it right before the program's first Convolution(2,2) — the
 * first operation that touches the stride-2 tables and the coarser levels' hash / rulebook / row counts, which the caller
 * may have built on another stream (they then overlap the level-0 operations in front of it). */
int sgnn_prog_forward(const int32_t *ops, const float *opf, int nops, const int32_t *bufs, int nbuf, int n_ext,
                      const int64_t *lev_n, const int64_t *lev_ld, void *const *lev_nbr,
                      void *const *lev_children, void *const *lev_ptable, void *const *lev_parent,
                      void *const *lev_cnt, int nlev, void *const *params, int nparams,
                      void *const *ext, void *const *idx, int nidx,
                      float *arena, int64_t arena_floats, const int32_t *keep, int training, void *wait_event,
                      void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_prog_backward(const int32_t *ops, const float *opf, int nops, const int32_t *bufs, int nbuf, int n_ext,
                       const int64_t *lev_n, const int64_t *lev_ld, void *const *lev_nbr,
                       void *const *lev_children, void *const *lev_ptable, void *const *lev_parent,
                       void *const *lev_cnt, int nlev, void *const *params, void *const *pgrads,
                       int nparams, void *const *ext,
                       void *const *gext, void *const *idx, int nidx, const float *arena, float *garena,
                       int64_t arena_floats, void *const *gout, const int32_t *keep, int training, void *ws,
                       int64_t ws_bytes, sgnn_stream_t stream);

/* Optional second lane for sgnn_prog_backward: every weight-gradient launch (dW + its reduce) runs on `stream2`
 * with workspace `ws2`, concurrently with the dX / BatchNorm chain on the caller's stream (both only read dy); the
 * call joins the lane before it returns control of the parameter gradients.  stream2 == NULL turns it off.
 * Process-wide setting; ws2 must be private to the lane and >= the largest sgnn_conv_bwd_weight_ws_bytes of the
 * program (smaller: the lane is silently not used). */
int sgnn_prog_set_side_stream(sgnn_stream_t stream2, void *ws2, int64_t ws2_bytes);
/* 1: sgnn_prog_backward no longer makes its stream wait for the weight-gradient lane at its end; the CALLER joins the
 * lane's stream before anything reads parameter gradients (train.GraphStep: once, before Adam).  A program's last weight
 * gradient — its first, widest convolution — otherwise holds up the next program's dependent chain for as long as it runs.
 * Returns the previous setting. */
int sgnn_prog_defer_join(int on);
/* ---------------------------------------------------------------------------
 * bf16 inference kernels (infer_bf16.hip; what sgnn_prog_forward runs with training = 2 | 4).  bf16 rows are uint16
 * bit patterns with a row stride ld* in ELEMENTS; fp32 math, one round-to-nearest-even per stored value.  Readers of
 * 16-byte row chunks (the convolutions) zero the channels >= cin in registers: pad columns may hold anything.
 * sgnn_bf16_conv_fwd: the rulebook walk of sgnn_conv_fwd (K = 27 submanifold / 8 stride-2, offset-major table, ld a
 *   multiple of 256) over bf16 rows with v_mfma_f32_16x16x32_bf16 (cin, cout <= 64; other widths: a plain generic
 *   kernel); fp32 weights (K, cin, cout) are rounded to bf16 into ws (sgnn_bf16_conv_ws_bytes(cin, cout, K, 0) bytes);
 *   optional bf16 residual `addend` added before the rounding; n_dev: capacity mode (rows past *n_dev untouched).
 *   ldx must be even and x dword-aligned.
 * sgnn_bf16_conv_expand: the 8-child up-sampling convolution (sgnn_conv_fwd_ex on the parent rulebook: child row
 *   8p + parity), from the 3x3x3 weights w; ws: sgnn_bf16_conv_ws_bytes(cin, cout, 27, 1) bytes.
 * sgnn_bf16_bn_eval: y = act((x - running_mean) / sqrt(running_var + eps) * gamma + beta), act = leaky ReLU (leak).
 * sgnn_bf16_gather_rows: y[r] = x[idx[r]] (UnPooling); sgnn_bf16_add: y = a + b; sgnn_bf16_join: y = [a | b].
 * sgnn_bf16_concat3: fp32 sources (contiguous, optional row indices, -1 = zeros) -> bf16 rows [a | b | c].
 * sgnn_bf16_linear: bf16 rows -> fp32 logits y[n][cout] (cout <= 4; w: cout x cin, bias: cout or NULL).
 * sgnn_bf16_to_f32: bf16 rows (stride ldx) -> contiguous fp32 [n][c].
 * ------------------------------------------------------------------------- */
int64_t sgnn_bf16_conv_ws_bytes(int cin, int cout, int K, int expand);
int sgnn_bf16_conv_fwd(const void *x, int64_t n_in, int cin, int64_t ldx, const float *w, int K, const int32_t *table,
                       int64_t ld, int64_t n_out, int cout, void *y, int64_t ldy, const void *addend, int64_t ld_add,
                       const int64_t *n_dev, void *ws, int64_t ws_bytes, sgnn_stream_t stream);
int sgnn_bf16_conv_expand(const void *x, int64_t n, int cin, int64_t ldx, const float *w, const int32_t *nbr, int64_t ld,
                          int cout, void *y, int64_t ldy, const int64_t *n_dev, void *ws, int64_t ws_bytes,
                          sgnn_stream_t stream);
int sgnn_bf16_bn_eval(const void *x, int64_t ldx, int64_t n, int c, const float *gamma, const float *beta,
                      const float *running_mean, const float *running_var, float eps, float leak, void *y, int64_t ldy,
                      const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_gather_rows(const void *x, int64_t ldx, int c, const int32_t *idx, int64_t m, void *y, int64_t ldy,
                          const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_add(const void *a, int64_t lda, const void *b, int64_t ldb, int64_t n, int c, void *y, int64_t ldy,
                  const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_join(const void *a, int64_t lda, int ca, const void *b, int64_t ldb, int cb, int64_t n, void *y, int64_t ldy,
                   const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_concat3(const float *a, int ca, const int32_t *ia, const float *b, int cb, const int32_t *ib, const float *c,
                      int cc, const int32_t *ic, int64_t m, void *y, int64_t ldy, const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_linear(const void *x, int64_t ldx, int64_t n, int cin, const float *w, const float *bias, int cout, float *y,
                     const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_to_f32(const void *x, int64_t ldx, int64_t n, int c, float *y, const int64_t *n_dev, sgnn_stream_t stream);
/* ---------------------------------------------------------------------------
 * Optimizer step (torch/train.py:81 optim.Adam, :264 optimizer.step()) as one launch over flat buffers of all n
 * parameters.  seg: HOST array of nseg (<= 8) x 5 int64 = {begin, end, cnt, flag, step}: elements [begin, end) are
 * updated iff the segment was reached this step — *flag > 0 (device float, if flag != 0), else *cnt > 0 (device
 * int64 row count, if cnt != 0), else always — which is torch.optim.Adam skipping parameters whose grad is None (a
 * generative stage without input sites, torch/model.py:211,260) decided on the device; step: device float counter
 * of the segment's updates (bias correction), incremented here.  lr_dev: device float.  grads are multiplied by
 * grad_scale (1 / world size after a sum all-reduce).  Nothing is updated while *status has SGNN_STATUS_OVERFLOW.
 * sgnn_seg_flags writes flags[t] = (*cnt_ptrs[t] > 0) for a data-parallel step's all-reduce (cnt_ptrs: HOST array of
 * device addresses, 0 = always 1) and, with status != NULL, flags[7] = this rank's overflow bit.
 * ------------------------------------------------------------------------- */
int sgnn_adam_flat(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *seg,
                   int nseg, const float *lr_dev, float beta1, float beta2, float eps, float weight_decay,
                   float grad_scale, const int32_t *status, sgnn_stream_t stream);
int sgnn_seg_flags(const int64_t *cnt_ptrs, int nseg, float *flags, const int32_t *status, sgnn_stream_t stream);
/* data parallel: flags[7] (written by sgnn_seg_flags from *status, summed by the all-reduce) > 0 -> raise
 * SGNN_STATUS_OVERFLOW locally, so that every replica discards the same step */
int sgnn_status_merge(const float *overflow_flag, int32_t *status, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * On-disk formats feeding the path: .sdfs training chunks, .sdf scenes, .knw masks.
 * Replaces torch/data_util.py:63-117 (load_train_file), :121-139 (load_scene), :142-155
 * (load_scene_known) and the mask + collate of torch/scene_dataloader.py:101-105, :13-36.
 *
 * sgnn_io_layout is host-only (no GPU needed): it validates one file image and returns the byte offset
 * and entry count of every section; nothing is copied.  kind: 0 .sdfs, 1 .sdf, 2 .knw.
 * out[24] (int64, -1 = section absent):
 *   [0..2] dimx, dimy, dimz   [3] voxelsize (f32 bit pattern)   [4] offset of world2grid (16 x f32)
 *   [5] n_input  [6] offset of its (x,y,z) u32 triples  [7] offset of its f32 values      (.sdf: the scene)
 *   [8] n_target [9] [10] likewise                                                         (.sdfs only)
 *   [11] offset of the u8 known volume (dimz*dimy*dimx bytes, z-major)                     (.sdfs, .knw)
 *   [12+3h .. 14+3h] count / triple offset / value offset of hierarchy level h, factor 2^(h+1) (.sdfs only)
 *   [21] bytes consumed
 * The device entry points work on a PACKED batch: the sections of all samples concatenated, with
 * seg[s] .. seg[s+1] delimiting sample s (device int64[nb+1]) and voxelsize[s] its voxel size.
 * ------------------------------------------------------------------------- */
int sgnn_io_layout(const void *bytes, int64_t nbytes, int kind, int64_t *out);
/* mask[i] = |value_i / voxelsize| < truncation && z_i < max_z   (scene_dataloader.py:83-86, :101) */
int sgnn_io_flag_entries(const uint32_t *locs_xyz, const float *vals, const float *voxelsize,
                         const int64_t *seg, int nb, int64_t n, float truncation, int64_t max_z,
                         uint8_t *mask, sgnn_stream_t stream);
/* rows j < *count: out_locs[j] = {z,y,x,sample} (int64), out_feats[j] = value/voxelsize of entry sel[j]
 * (sel from sgnn_compact_mask: ascending, so file order is kept as collate keeps it) */
int sgnn_io_emit_entries(const uint32_t *locs_xyz, const float *vals, const float *voxelsize,
                         const int64_t *seg, int nb, const int32_t *sel, const int64_t *count,
                         int64_t n_max, int64_t *out_locs, float *out_feats, sgnn_stream_t stream);
/* dense[s][z][y][x] = value/voxelsize (data_util.py:44-56 sparse_to_dense_np); `dense` is (nb,d0,d1,d2)
 * pre-filled by the caller (-inf); entries outside the volume or with z >= max_z are skipped */
int sgnn_io_scatter_dense(const uint32_t *locs_xyz, const float *vals, const float *voxelsize,
                          const int64_t *seg, int nb, int64_t n, int d0, int d1, int d2, int64_t max_z,
                          float *dense, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * TSDF fusion: depth frames -> scan volume -> .sdf / .knw blocks or the collated scene input (the step of
 * datagen/GenerateScans that produces the files above; rules in INTEGRATION.md "TSDF fusion").
 * Volumes are dense (dz, dy, dx) arrays, x fastest: sdf f32 in metres (-inf = never observed), weight u8,
 * free counter i32.  Depth frames are one (nframes, h, w) f32 stack in metres, -inf = invalid.
 * ------------------------------------------------------------------------- */
/* one frame of sgnn_fuse_integrate (96 bytes; the frame table is a device array of these) */
typedef struct sgnn_fuse_frame {
  float m[12];    /* rows 0..2 of inv(cam2world) * inv(world2grid): voxel (i,j,k,1) -> camera, fp32 */
  float intr[4];  /* fx, fy, cx, cy */
  int32_t box[6]; /* frustum box in voxels, inclusive: x0, x1, y0, y1, z0, z1 (empty when x0 > x1 or ...) */
  int64_t offset; /* element offset of this frame's (h, w) image in the depth stack */
} sgnn_fuse_frame;
/* out[f][j][i] = metric depth of raw[f] (nframes, h_raw, w_raw) u16 resampled to (h, w) by nearest index
 * round(i * (w_raw-1)/(w-1)): (1/depth_shift) * d, -inf where d == 0 or outside [min_depth, max_depth] */
int sgnn_fuse_depth_raw(const uint16_t *raw, int nframes, int h_raw, int w_raw, int h, int w, float depth_shift,
                        float min_depth, float max_depth, float *out, sgnn_stream_t stream);
/* bilateral filter of every frame (radius ceil(2 sigma_d)); in and out must not alias */
int sgnn_fuse_bilateral(const float *in, int nframes, int h, int w, float sigma_d, float sigma_r, float *out,
                        sgnn_stream_t stream);
/* integrate frames 0..nframes-1 in order into (sdf, weight, free_ctr), `chunk` frames per launch (<= 0: all; the
 * result does not depend on it).  obb: host float[12] = corner a, edges e0, e1, e2 in voxel coordinates, or NULL */
int sgnn_fuse_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, int dx, int dy, int dz, const float *depth,
                        int h, int w, const sgnn_fuse_frame *frames, int nframes, int chunk, float voxel_size,
                        float depth_min, float depth_max, const float *obb, sgnn_stream_t stream);
/* mask[v] = |sdf[v]| <= keep_abs, and — truncation > 0 — |sdf[v] / voxel_size| < truncation and z < max_z */
int sgnn_fuse_flag(const float *sdf, int dx, int dy, int dz, float keep_abs, float truncation, float voxel_size,
                   int64_t max_z, uint8_t *mask, sgnn_stream_t stream);
/* rows q < *count (sel from sgnn_compact_mask of the flags): locs_xyz[q] = (x, y, z) u32 and vals[q] = sdf, the
 * layout of an .sdf block */
int sgnn_fuse_emit_block(const float *sdf, int dx, int dy, const int32_t *sel, const int64_t *count, int64_t n_max,
                         uint32_t *locs_xyz, float *vals, sgnn_stream_t stream);
/* the same as collated scene input: locs[q] = {z, y, x, 0} int64, feats[q] = sdf / voxel_size */
int sgnn_fuse_emit_rows(const float *sdf, int dx, int dy, float voxel_size, const int32_t *sel, const int64_t *count,
                        int64_t n_max, int64_t *locs, float *feats, sgnn_stream_t stream);
/* u8 known codes of the .knw file: sdf < -vs -> max(2, min(255, (int)(-sdf/vs) + 1)), sdf <= vs -> 1, else 0;
 * -inf -> 2 */
int sgnn_fuse_known(const float *sdf, int64_t n, float voxel_size, uint8_t *known, sgnn_stream_t stream);
/* Colour (rules in INTEGRATION.md section M).  Colour frames are one (nframes, h, w, 4) u8 stack, memory order R, G, B,
 * A, on the pixel grid of the depth stack; A != 0 = the pixel has a colour.  The colour state of a volume is one
 * (dz, dy, dx, 4) u16 array, 8-byte aligned: R, G, B in 8.8 fixed point and the colour weight 0..255, zero at the start.
 * out = raw (nframes, h_raw, w_raw, channels = 3 | 4) u8 resampled to (h, w) by sgnn_fuse_depth_raw's nearest index;
 * A = 255 for 3 channels, (a != 0) ? 255 : 0 for 4 */
int sgnn_fusecol_pack(const uint8_t *raw, int nframes, int h_raw, int w_raw, int channels, int h, int w, uint8_t *out,
                      sgnn_stream_t stream);
/* sgnn_fuse_integrate that also folds rgba into color: same geometry result bit for bit; a sample that updates the
 * geometry, was not clamped on the free-space side and whose pixel has A != 0 updates the voxel's colour */
int sgnn_fusecol_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, uint16_t *color, int dx, int dy, int dz,
                           const float *depth, const uint8_t *rgba, int h, int w, const sgnn_fuse_frame *frames,
                           int nframes, int chunk, float voxel_size, float depth_min, float depth_max,
                           const float *obb, sgnn_stream_t stream);
/* rgb (n, 3) u8 = (q + 128) >> 8 where the colour weight is positive, else 0; wc (n) u8 = the colour weight, or NULL.
 * rgb and wc 4-byte aligned */
int sgnn_fusecol_export(const uint16_t *color, int64_t n, uint8_t *rgb, uint8_t *wc, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Training chunks cut from a fused scan pair (sgnn_amd.chunks; rules in INTEGRATION.md "Training chunks"): window
 * scores, and the collated batch of B crops of an input volume and a target pyramid, without .sdfs files.
 * Volumes are the dense (dz, dy, dx) f32 arrays of the fusion above.  origins: device int32 (nb, 3) = z, y, x of each
 * crop in FINE voxels; crop extents (cz, cy, cx) are in voxels of the level at hand, cx a multiple of 4.  A window
 * may reach past the volume: out there nothing is read, the input has no sites, dense values are -inf, known is 255.
 * ------------------------------------------------------------------------- */
/* table[w] = {voxels of the window with |sdf_target / vs| < truncation, voxels with |sdf_input| <= keep_abs and
 * |sdf_input / vs| < truncation} (int32 pairs), window w = (wz * nwy + wy) * nwx + wx at origin (wz*sz, wy*sy, wx*sx)
 * with extent (cz, cy, cx); extents and strides are multiples of 8.  bricks: workspace of
 * 2 * ceil(dz/8) * ceil(dy/8) * ceil(dx/8) int32 (the per-brick counts, summed into windows by a second kernel).
 * Integer sums only: the table is exact and does not depend on any order. */
int sgnn_chunk_score(const float *sdf_target, const float *sdf_input, int dx, int dy, int dz, float voxel_size,
                     float truncation, float keep_abs, int cz, int cy, int cx, int sz, int sy, int sx, int nwz, int nwy,
                     int nwx, int32_t *bricks, int32_t *table, sgnn_stream_t stream);
/* mask[((b * cz + z) * cy + y) * cx + x] = voxel origin_b + (z, y, x) is inside the volume and |sdf| <= keep_abs and
 * |sdf / voxel_size| < truncation (the filters of sgnn_fuse_flag) */
int sgnn_chunk_flag(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz, int cy, int cx,
                    float keep_abs, float truncation, float voxel_size, uint8_t *mask, sgnn_stream_t stream);
/* rows q < *count (sel from sgnn_compact_mask of that mask): locs[q] = {z, y, x, b} int64 relative to the crop origin,
 * feats[q] = sdf / voxel_size */
int sgnn_chunk_emit_rows(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz, int cy,
                         int cx, float voxel_size, const int32_t *sel, const int64_t *count, int64_t n_max,
                         int64_t *locs, float *feats, sgnn_stream_t stream);
/* out (nb, cz, cy, cx) f32 = (sdf / 2^shift) / voxel_size where |sdf| <= keep_abs, else -inf, read from a volume of
 * pyramid level `shift` at origin_b >> shift; voxel_size is the FINE voxel size (the divisor of the file loaders).
 * known (nb, cz, cy, cx) u8 or NULL: the .knw codes of sgnn_fuse_known at voxel_size, 255 outside the volume.
 * One launch for all nb crops. */
int sgnn_chunk_crop(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz, int cy, int cx,
                    int shift, float keep_abs, float voxel_size, float *out, uint8_t *known, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Depth frames rendered from a triangle mesh (sgnn_amd.render; rules in INTEGRATION.md section F): the virtual-scan
 * source of datagen/GenerateScans (Scene.cpp:107-158).  The output is what sgnn_fuse_bilateral / sgnn_fuse_integrate
 * take: one (nframes, h, w) f32 stack in metres, -inf = nothing seen.
 * ------------------------------------------------------------------------- */
/* one frame of sgnn_render_depth (64 bytes; the frame table is a device array of these) */
typedef struct sgnn_render_frame {
  float m[12];   /* rows 0..2 of inv(cam2world): world (x,y,z,1) -> camera, fp32; NaN = non-finite pose, empty frame */
  float intr[4]; /* fx, fy, cx, cy */
} sgnn_render_frame;
/* verts (nverts, 3) f32 world metres, faces (ntri, 3) i32, out (nframes, h, w) f32, 16-byte aligned; the output is
 * the depth buffer while the call runs.  chunk: frames per triangle launch (<= 0: all), wave_pixels: pixel boxes
 * above it are rasterised by a whole wave (<= 0: the built-in constant); the result depends on neither.  A face
 * with an index outside [0, nverts) is not drawn and, with status != NULL, raises SGNN_STATUS_COORD_RANGE there.
 * counters: NULL, or device int64[3] that the call adds to (measurements and tests): triangles drawn by one lane,
 * triangles drawn by a wave, covered pixels (= atomic minima issued).  h, w <= 16384; ntri * 3 and
 * nframes * h * w < 2^31. */
int sgnn_render_depth(const float *verts, int nverts, const int32_t *faces, int ntri, const sgnn_render_frame *frames,
                      int nframes, int chunk, int h, int w, float z_clip, float depth_min, float depth_max,
                      int wave_pixels, float *out, int32_t *status, int64_t *counters, sgnn_stream_t stream);
/* Colour frames with the depth (rules in INTEGRATION.md section N): sgnn_render_depth of a mesh whose vertices carry
 * a colour, vcolors (nverts, 3) u8 R, G, B.  out is the depth stack of sgnn_render_depth, bit for bit; rgba
 * (nframes, h, w, 4) u8, memory order R, G, B, A, 4-byte aligned, is the colour stack sgnn_fusecol_integrate takes:
 * A = 255 where out is finite, (0, 0, 0, 0) elsewhere.  The colour is interpolated perspective-correctly; among
 * fragments of equal depth the smallest R<<24 | G<<16 | B<<8 wins.  keys: workspace of nframes * h * w u64, 16-byte
 * aligned, the depth buffer while the call runs (z bits in the high word, the colour in the low word, folded with
 * one 64-bit unsigned atomic minimum per covered pixel). */
int sgnn_rendercol_draw(const float *verts, int nverts, const int32_t *faces, int ntri, const sgnn_render_frame *frames,
                        int nframes, int chunk, int h, int w, float z_clip, float depth_min, float depth_max,
                        int wave_pixels, float *out, int32_t *status, int64_t *counters, const uint8_t *vcolors,
                        uint64_t *keys, uint8_t *rgba, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mesh-to-mesh distances (sgnn_amd.meshdist; rules in INTEGRATION.md section G): the exact nearest triangle of a
 * mesh for many query points through a uniform grid of triangle lists, and area-weighted surface samples.
 *   sgnn_meshdist_pack   -> records (ntri, 12) f32: a, ab, ac as three 16-byte rows (w = 0); boxes (ntri, 6) f32:
 *                           min and max corner of the face; usable (ntri) u8.  A face that rule 1 ignores gets the
 *                           box (+inf, -inf), which the passes below skip.  An index outside [0, nverts) makes the
 *                           face unusable and, with status != NULL, raises SGNN_STATUS_COORD_RANGE there.
 *   sgnn_meshdist_count  -> counts[cell] += faces whose box touches the cell (the caller zeroes counts)
 *   (caller: offsets = exclusive scan of counts, nx*ny*nz + 1 entries, i32; the total must stay below 2^31)
 *   sgnn_meshdist_fill   -> refs[offsets[cell] + k] = face, k from the zeroed cursor array; order inside a list is
 *                           arbitrary and does not show in any result
 *   sgnn_meshdist_query  -> dist (npts) f32 and face (npts) i32 by the shell walk of rule 5; max_dist = +inf for an
 *                           unbounded query.  counters: NULL, or device int64[2] that the call adds to: cells
 *                           visited, (point, face) pairs evaluated.
 *   sgnn_mesh_sample     -> pts (n, 3) f32 and fid (n) i32 of rule 6 from the records and the fp64 cumulative areas
 *                           cum (ntri); last_usable = the face a search past the end is clamped to.
 * The grid is lo (3 floats), hi (3 floats, query only), pitch cell > 0 and nx, ny, nz cells, nx*ny*nz < 2^31.
 * ------------------------------------------------------------------------- */
int sgnn_meshdist_pack(const float *verts, int nverts, const int32_t *faces, int ntri, float *records, float *boxes,
                       uint8_t *usable, int32_t *status, sgnn_stream_t stream);
int sgnn_meshdist_count(const float *boxes, int ntri, float lox, float loy, float loz, float cell, int nx, int ny,
                        int nz, int32_t *counts, sgnn_stream_t stream);
int sgnn_meshdist_fill(const float *boxes, int ntri, float lox, float loy, float loz, float cell, int nx, int ny,
                       int nz, const int32_t *offsets, int32_t *cursor, int32_t *refs, sgnn_stream_t stream);
int sgnn_meshdist_query(const float *points, int64_t npts, const float *records, const int32_t *offsets,
                        const int32_t *refs, float lox, float loy, float loz, float hix, float hiy, float hiz,
                        float cell, int nx, int ny, int nz, float max_dist, float *dist, int32_t *face,
                        int64_t *counters, sgnn_stream_t stream);
int sgnn_mesh_sample(const float *records, const double *cum, int ntri, int last_usable, int64_t n, int64_t seed,
                     float *pts, int32_t *fid, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * TSDF volumes ray-cast to depth and normal frames (sgnn_amd.raycast; rules in INTEGRATION.md section H): the way
 * back from a volume to images, at the camera conventions of the fusion and render blocks above.  The volume is a
 * dense (dz, dy, dx) f32 array in any unit, band in the same unit: a voxel is usable iff |sdf| < band (never for a
 * NaN or an infinity).  The output is what sgnn_fuse_bilateral / sgnn_fuse_integrate take: one (nframes, h, w) f32
 * stack of z-depths, -inf = no hit.
 * ------------------------------------------------------------------------- */
/* one frame of the cast below (64 bytes; the frame table is a device array of these) */
typedef struct sgnn_raycast_frame {
  float g[12];   /* rows 0..2 of world2grid . cam2world: camera (x,y,z,1) -> voxel coordinates, fp32; NaN = empty frame */
  float intr[4]; /* fx, fy, cx, cy */
} sgnn_raycast_frame;
/* bricks[(bz * nby + by) * nbx + bx] = 1 iff the 8x8x8 brick holds a usable voxel, else 0; nb? = ceil(d? / 8),
 * d? <= 65535 */
int sgnn_raycast_bricks(const float *sdf, int dx, int dy, int dz, float band, uint8_t *bricks, sgnn_stream_t stream);
/* depth (nframes, h, w) f32 and, with normal != NULL, normal (nframes, h, w, 3) f32 in camera space (NaN = none).
 * Samples sit at depth_min + (float)k * dt for k < nsamples (<= 2^20).  bricks: the table of the pass above for the
 * same volume and band, or NULL to visit every sample; chunk: frames per launch (<= 0: all); the result depends on
 * neither.  counters: NULL, or device int64[2] that the call adds to (measurements and tests): samples put through
 * the range test and the eight corner fetches, samples passed over through the brick table.
 * nframes * h * w < 2^31. */
int sgnn_raycast_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                      const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w, float depth_min, float dt,
                      int nsamples, float *depth, float *normal, int64_t *counters, sgnn_stream_t stream);
/* Colour frames with the depth (rules in INTEGRATION.md section N): sgnn_raycast_cast of a volume that also has a
 * colour per voxel, colors (dz, dy, dx, 4) u8 R, G, B, A, 4-byte aligned, A != 0 = the voxel has a colour.  depth and
 * normal are those of sgnn_raycast_cast, bit for bit; rgba (nframes, h, w, 4) u8, 4-byte aligned: at a hit the
 * weighted mean of the coloured corners of the hit's cell with A = 255, (0, 0, 0, 0) for no hit or no coloured
 * corner.  Only a ray with a hit reads colours. */
int sgnn_raycol_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                     const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w, float depth_min, float dt,
                     int nsamples, float *depth, float *normal, int64_t *counters, const uint8_t *colors, uint8_t *rgba,
                     sgnn_stream_t stream);
/* The differentiable cast (sgnn_amd.raycast.cast_diff; rules in INTEGRATION.md section U).  The forward is
 * sgnn_raycast_cast without normals and counters, depth bit for bit, and it also writes hit (nframes, h, w) i32, the
 * sample index k of each pixel's hit (the valid sample <= 0; the previous one is k - 1), -1 = no hit; ok
 * (nframes, h, w) u8, 1 iff the pixel has a hit whose own cell lies in the volume with eight usable corners; and,
 * with features (dz, dy, dx, channels) f32, 1 <= channels <= 16, feat (nframes, h, w, channels) f32: the trilinear
 * weighted sum of all eight corners' features at the hit, 0 where there is no hit or the cell test fails.  features
 * and feat are both NULL (channels 0) or both given. */
int sgnn_raygrad_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                      const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w, float depth_min, float dt,
                      int nsamples, const float *features, int channels, float *depth, int32_t *hit, float *feat,
                      uint8_t *ok, sgnn_stream_t stream);
/* Its backward: from hit (the forward's record for the same volume, frames and samples) and the incoming gradients
 * grad_depth (nframes, h, w) and grad_feat (nframes, h, w, channels), either of which may be NULL (zero), ADDS the
 * gradients into caller-zeroed grad_sdf (dz, dy, dx) and grad_features (dz, dy, dx, channels) with fp32 atomic adds;
 * either may be NULL (not wanted).  features NULL (channels 0) takes NULL grad_feat and grad_features.  A pixel
 * without a hit adds nothing and its incoming gradient is not read; a record that names no crossing inside the
 * volume adds nothing either. */
int sgnn_raygrad_backward(const float *sdf, int dx, int dy, int dz, const sgnn_raycast_frame *frames, int nframes,
                          int chunk, int h, int w, float depth_min, float dt, int nsamples, const int32_t *hit,
                          const float *features, int channels, const float *grad_depth, const float *grad_feat,
                          float *grad_sdf, float *grad_features, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Depth frames tracked against a volume (sgnn_amd.track; rules in INTEGRATION.md section I): the "frame to model"
 * half that goes with the cast above.  One Gauss-Newton system of projective point-to-plane ICP per (live frame,
 * model frame) pair, the depth pyramid and the live normals; the 6x6 solve and the pose update stay on the host.
 * Frames are (n, h, w) f32 z-depths, -inf = no depth, at the camera conventions of the blocks above; the model
 * depth and normal frames are what sgnn_raycast_cast writes.
 * ------------------------------------------------------------------------- */
/* one (live frame, model frame) pair of sgnn_track_system (96 bytes; the pair table is a device array of these) */
typedef struct sgnn_track_pair {
  float t[12];         /* rows 0..2 of T = inv(model cam2world) . live cam2world: live camera (x,y,z,1) -> model
                          camera, fp32; NaN = non-finite pose, empty system */
  float intr_live[4];  /* fx, fy, cx, cy of the live frame */
  float intr_model[4]; /* fx, fy, cx, cy of the model frame */
  float pad[4];
} sgnn_track_pair;
#define SGNN_TRACK_MAX_BLOCKS 256 /* partial sums per pair that sgnn_track_system keeps in its workspace */
/* out (nframes, h/2, w/2) f32: per 2x2 block the mean of the finite values within delta of the smallest finite one
 * (rule 9), -inf if none.  nframes * h * w < 2^31; an empty output (h or w of 1, no frame) launches nothing. */
int sgnn_track_halve(const float *depth, int nframes, int h, int w, float delta, float *out, sgnn_stream_t stream);
/* normal (nframes, h, w, 3) f32: camera-space unit normals of a depth frame from its four axis neighbours (rule 10),
 * facing the camera, NaN = none.  intr (nframes, 4) f32 on the device: fx, fy, cx, cy.  nframes * h * w < 2^31. */
int sgnn_track_normals(const float *depth, const float *intr, int nframes, int h, int w, float delta, float *normal,
                       sgnn_stream_t stream);
/* out (npairs, 32) f64: per pair the 21 sums of the upper triangle of J^T J (row-major), the 6 of J^T r, the sum of
 * r^2, the number of associated pixels, and three zeros (rules 2-6).  depth (npairs, h, w); live_normal (npairs, h,
 * w, 3) or NULL (no angle gate); model_depth (npairs, hm, wm) and model_normal (npairs, hm, wm, 3).  max_dist2: the
 * squared distance gate, cos_min: the angle gate, both rounded by the caller.  residual (npairs, h, w) f32 (NaN = no
 * association) and assoc (npairs, h, w) i32 (v * wm + u, or -1) may be NULL.  ws: at least npairs *
 * min(ceil(h * w / 256), SGNN_TRACK_MAX_BLOCKS) * 256 bytes; the number of partial sums depends on (h, w) alone and
 * they are added in index order, so neither npairs nor the launch shows in any bit of the result.
 * npairs <= 65535; npairs * h * w and npairs * hm * wm < 2^31. */
int sgnn_track_system(const float *depth, const float *live_normal, int h, int w, const float *model_depth,
                      const float *model_normal, int hm, int wm, const sgnn_track_pair *pairs, int npairs,
                      float max_dist2, float cos_min, double *out, float *residual, int32_t *assoc, void *ws,
                      int64_t ws_bytes, sgnn_stream_t stream);
/* Tracking with colour (rules in INTEGRATION.md section T).
 * out (n) f32: the intensity (77 R + 150 G + 29 B) / 256 of n R, G, B, A pixels, NaN where A == 0 (rule T1).
 * n < 2^31 - 256. */
int sgnn_track_intensity(const uint8_t *rgba, int64_t n, float *out, sgnn_stream_t stream);
/* out (nframes, h/2, w/2) f32: per 2x2 block the mean intensity of the pixels that sgnn_track_halve averages at the
 * same delta and whose intensity is not NaN, NaN if none (rule T2).  Sizes as sgnn_track_halve. */
int sgnn_track_halve_intensity(const float *depth, const float *intensity, int nframes, int h, int w, float delta,
                               float *out, sgnn_stream_t stream);
/* out (npairs, 32) f64 in the layout of sgnn_track_system: the photometric system of the live pixels that pass that
 * call's gates (same pairs, max_dist2, cos_min and live_normal) and rule T3's.  live_intensity (npairs, h, w) and
 * model_intensity (npairs, hm, wm) f32, NaN = none; max_dist: the gate on the four corner depths, metres;
 * max_intensity: the gate on |r|.  residual (npairs, h, w) f32 (model minus live intensity, NaN = none) and cell
 * (npairs, h, w) i32 (y0 * wm + x0 of the bilinear cell, or -1) may be NULL.  Workspace, limits and the fixed order
 * of the additions as sgnn_track_system. */
int sgnn_track_color_system(const float *depth, const float *live_normal, const float *live_intensity, int h, int w,
                            const float *model_depth, const float *model_normal, const float *model_intensity, int hm,
                            int wm, const sgnn_track_pair *pairs, int npairs, float max_dist2, float cos_min,
                            float max_dist, float max_intensity, double *out, float *residual, int32_t *cell, void *ws,
                            int64_t ws_bytes, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Point sets registered against a volume (sgnn_amd.register; rules in INTEGRATION.md section R): point-to-SDF
 * Gauss-Newton.  The residual of a source point is the trilinear sample of the destination's sdf at its transformed
 * position, its Jacobian the gradient of the same interpolant; the system has the layout of sgnn_track_system, and
 * the 6x6 solve and the update of the transform stay on the host.
 * ------------------------------------------------------------------------- */
/* one transform of sgnn_register_system (96 bytes; the record table is a device array of these) */
typedef struct sgnn_register_pair {
  float t[12]; /* rows 0..2 of T: source world (x,y,z,1) -> destination world, fp32; NaN = non-finite record, empty
                  system */
  float w[12]; /* rows 0..2 of the destination's world2grid: world (x,y,z,1) -> voxel coordinates, fp32 */
} sgnn_register_pair;
#define SGNN_REGISTER_MAX_BLOCKS 256 /* partial sums per record that sgnn_register_system keeps in its workspace */
/* out (npairs, 32) f64: per record the 21 sums of the upper triangle of J^T J (row-major), the 6 of J^T r, the sum of
 * r^2, the number of associated points, and three zeros (rules 2-7).  points (npoints, 3) f32 in the source world; sdf
 * (dz, dy, dx) f32 of the destination in any unit, band and max_dist in the same unit; min_grad2: the smallest squared
 * length of the world-space gradient an association may have, rounded by the caller.  Every record runs against the
 * same points and the same volume.  residual (npairs, npoints) f32 (NaN = no association) and cell (npairs, npoints)
 * i32 ((fz * dy + fy) * dx + fx of the sample's cell, or -1) may be NULL.  ws: at least npairs *
 * min(ceil(npoints / 256), SGNN_REGISTER_MAX_BLOCKS) * 256 bytes; the number of partial sums depends on npoints alone
 * and they are added in index order, so neither npairs nor the launch shows in any bit of the result.
 * npoints < 2^31 - 65536; npairs <= 65535; dx, dy, dz >= 2 and dx * dy * dz < 2^31; band, max_dist > 0;
 * min_grad2 >= 0.  npoints == 0 or npairs == 0 launches nothing and writes nothing. */
int sgnn_register_system(const float *points, int npoints, const float *sdf, int dx, int dy, int dz,
                         const sgnn_register_pair *pairs, int npairs, float band, float max_dist, float min_grad2,
                         double *out, float *residual, int32_t *cell, void *ws, int64_t ws_bytes,
                         sgnn_stream_t stream);

/* Candidate transforms scored against an integer distance field (register.search; rules in INTEGRATION.md section X).
 * One candidate of sgnn_register_score (48 bytes; the record table is a device array of these): */
typedef struct sgnn_register_pose {
  float m[12]; /* rows 0..2 of world2grid . T: source world (x,y,z,1) -> voxel coordinates of the field, formed in fp64
                  and rounded to fp32 by the caller; NaN = non-finite record, every point outside */
} sgnn_register_pose;
#define SGNN_REGISTER_SCORE_MAX_POSES (1 << 24) /* records of one sgnn_register_score call */
/* out (nposes, 3) i64, written in full by the call: per record the cost, the inliers and the points outside.  points
 * (npoints, 3) f32 in the source world, shared by all records; dist2 (dz, dy, dx) i32: squared distances in voxels, -1 =
 * nothing within reach (sgnn_edt_axis' dist2).  A point goes to voxel n = floor(g + 0.5f) per axis of g = m . p; it is
 * outside where g is not finite or 0 <= n <= d - 1 fails, tested in float.  An outside point costs cap2; one inside
 * costs cap2 where dist2[n] < 0, else min(dist2[n], cap2), and is an inlier where 0 <= dist2[n] <= inlier2.  The sums
 * are exact integers: no bit depends on nposes, on the launch or on the order of the additions.
 * npoints < 2^31 - 65536; nposes <= SGNN_REGISTER_SCORE_MAX_POSES; dx, dy, dz >= 1 and dx * dy * dz < 2^31; cap2 > 0;
 * inlier2 >= 0.  npoints == 0 writes zeros; nposes == 0 launches nothing and writes nothing. */
int sgnn_register_score(const float *points, int npoints, const int32_t *dist2, int dx, int dy, int dz,
                        const sgnn_register_pose *poses, int nposes, int cap2, int inlier2, int64_t *out,
                        sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * The gravity-aligned room frame of a volume (sgnn_amd.upright; rules in INTEGRATION.md section S): votes of the
 * surface normals of a TSDF volume.  A surface voxel is an interior voxel whose sdf and six axis neighbours are finite
 * with |.| < band and whose own |sdf| < surface; its normal is the central difference taken to the world through the
 * transpose of world2grid's 3x3 (rule S.1).  The three entry points walk the same voxels: sdf (dz, dy, dx) f32 on the
 * device, dx * dy * dz < 2^31, band and surface > 0 in the sdf's unit; world2grid (and grid2world, its inverse as the
 * caller rounded it): 12 finite floats on the host, rows 0..2.  Every output is an integer count or a 2^20 fixed-point
 * integer sum that the call adds into (the caller zeroes it), so neither the launch nor the order of the atomics
 * shows in any bit.  A volume with a dimension below 3 has no interior voxel: nothing is launched or written.  The
 * peak search, the cone iteration, the yaw and the floor level stay on the host.
 * ------------------------------------------------------------------------- */
/* one candidate axis of sgnn_upright_sums (48 bytes; the record table is a device array of these); a non-finite entry
 * makes the record empty */
typedef struct sgnn_upright_axis {
  float u[3];     /* the axis, unit length */
  float e1[3];    /* two unit vectors that span the plane normal to u: the frame the wall angle is measured in */
  float e2[3];
  float cos_cone; /* a normal n votes for the axis when |n . u| >= cos_cone */
  float sin_wall; /* a normal n is a wall normal when |n . u| <= sin_wall */
  float pad[1];
} sgnn_upright_axis;
#define SGNN_UPRIGHT_MAX_HEIGHT_BINS 4096 /* the most bins per row of sgnn_upright_heights */
/* hist (6, bins, bins) i32: the cube-map histogram of the unnormalised normals (rule S.2), bin (f * bins + iv) * bins +
 * iu with f = 2 * major axis + (negative).  bins is 8, 16 or 32. */
int sgnn_upright_histogram(const float *sdf, int dx, int dy, int dz, const float *world2grid, float band, float surface,
                           int bins, int32_t *hist, sgnn_stream_t stream);
/* out (nrecords, 8) i64 (rule S.4): per record the 2^20 fixed-point sums of sign(n . u) n over the normals inside the
 * cone (x, y, z), the number of those with n . u > 0 and with n . u < 0, the 2^20 fixed-point sums of cos 4a and sin 4a
 * of the wall normals' angle a in the (e1, e2) frame, and the number of wall normals.  records: device array; every
 * record runs against the same volume in one launch.  nrecords <= 65535; 0 launches nothing. */
int sgnn_upright_sums(const float *sdf, int dx, int dy, int dz, const float *world2grid, float band, float surface,
                      const sgnn_upright_axis *records, int nrecords, int64_t *out, sgnn_stream_t stream);
/* hist (2, nbins) i32 (rule S.5): heights h = (p - v n) . up of the surface voxels carried to the zero crossing along
 * their normals, bin floor((h - h0) / bin), voxels outside [0, nbins) dropped; row 0 the normals with n . up >=
 * cos_cone (floors), row 1 those with n . up <= -cos_cone (ceilings).  up: 3 finite floats on the host.  cos_cone > 0, bin > 0;
 * 1 <= nbins <= SGNN_UPRIGHT_MAX_HEIGHT_BINS. */
int sgnn_upright_heights(const float *sdf, int dx, int dy, int dz, const float *world2grid, const float *grid2world,
                         float band, float surface, const float *up, float cos_cone, float h0, float bin, int nbins,
                         int32_t *hist, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * A depth sensor simulated on rendered frames (sgnn_amd.sensor; rules in INTEGRATION.md section V): clean metric
 * z-depth in, what a structured-light sensor with a horizontal baseline would have returned out.  Frames are (nframes,
 * h, w) f32 on the device, -inf = no data, at the camera conventions of the blocks above; intrinsics (nframes, 4) f32
 * on the device: fx, fy, cx, cy per frame, finite, fx and fy not 0 (the caller checks).  nframes * h * w < 2^31;
 * nframes * h * w == 0 launches nothing and writes nothing.  Every result is a function of the pixel, its frame id and
 * the seed alone: neither the launch nor the way frames are split over calls shows in any bit.
 * ------------------------------------------------------------------------- */
/* the sensor of sgnn_sensor_degrade (48 bytes, read on the host); a stage is off at the value named */
typedef struct sgnn_sensor_model {
  float lateral_sigma;     /* V.3: standard deviation in pixels of the lateral jitter, >= 0; 0 = off */
  float min_depth;         /* V.4: a source depth below min_depth or above max_depth is no data; -inf, +inf = off */
  float max_depth;
  float baseline;          /* V.5, V.9: the projector sits at (baseline, 0, 0) in the camera frame, metres; 0 = no
                              shadow and no disparity steps */
  float cos_min;           /* V.6: a pixel whose incidence angle has a cosine below cos_min is dropped, [0, 1]; 0 = off */
  float edge_drop;         /* V.6: the share of edge pixels that are dropped, [0, 1]; 0 = off */
  float drop;              /* V.7: the share of all pixels that are dropped, [0, 1]; 0 = off */
  float a0;                /* V.8: sigma = (a0 + a1 (z - a2)^2) (1 + a3 tan^2(incidence)), metres; a0 = a1 = 0 = off */
  float a1;
  float a2;
  float a3;
  float disparity_quantum; /* V.9: the step of the disparity fx |baseline| / z in pixels, >= 0; 0 = off */
} sgnn_sensor_model;
/* mask (nframes, h, w) u8: 1 where a pixel with finite depth > 0 is hidden from the projector by a pixel of its own
 * row (rule V.5: for baseline > 0, some valid pixel x2 > x has projector column x2 - fx baseline / z2 <= that of x;
 * for baseline < 0 the mirror image), 0 elsewhere; all 0 for baseline == 0.  baseline finite. */
int sgnn_sensor_shadow(const float *depth, int nframes, int h, int w, const float *intrinsics, float baseline,
                       uint8_t *mask, sgnn_stream_t stream);
/* out (nframes, h, w) f32, not depth itself: rules V.1 - V.9 per pixel.  mask: what sgnn_sensor_shadow wrote for the
 * same depth, intrinsics and m->baseline; may be NULL when m->baseline == 0.  frame_ids (nframes) i64 on the device:
 * the frame number that enters the random draws of each frame (rule V.1), NULL = 0 .. nframes - 1.  m: on the host;
 * a field outside the range its comment names is SGNN_EINVAL. */
int sgnn_sensor_degrade(const float *depth, const uint8_t *mask, int nframes, int h, int w, const float *intrinsics,
                        const int64_t *frame_ids, const sgnn_sensor_model *m, uint64_t seed, float *out,
                        sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Arbitrary rays against a triangle mesh (sgnn_amd.raytrace; rules in INTEGRATION.md section W): the closest hit of
 * every ray, or whether anything lies on a segment.  The mesh is the index of the mesh-distance block above: records
 * from sgnn_meshdist_pack, offsets / refs from sgnn_meshdist_count / fill run on boxes grown by `guard` on every side
 * (rule W.4), over the grid lo (3 floats), pitch cell > 0, nx, ny, nz cells (nx*ny*nz < 2^31), all finite, guard >= 0.
 * origins, dirs (nrays, 3) f32; a ray is origin + t dir, dir is used as given (not normalised).  A face is hit iff the
 * test of rule W.1 passes with t_min < t < t_max (t_min finite); cull_back (0 or 1) = 1 keeps faces with det > 0 only.
 * counters: NULL, or device int64[2] that the call adds to: cells visited, (ray, face) pairs tested.
 *   sgnn_raytrace_closest  -> t (nrays) f32, face (nrays) i32, uv (nrays, 2) f32 of the smallest t over all usable
 *                             faces, the lowest face index among equal t; a miss is +inf, -1, (0, 0).  t_min < t_max.
 *   sgnn_raytrace_occluded -> hit (nrays) u8: 1 iff some usable face is hit within (t_min, t_max[ray]); t_max (nrays)
 *                             f32 on the device, a ray whose t_max is not above t_min is a miss.
 * A ray with a non-finite component or a zero direction is a miss.
 * ------------------------------------------------------------------------- */
int sgnn_raytrace_closest(const float *origins, const float *dirs, int64_t nrays, float t_min, float t_max,
                          const float *records, const int32_t *offsets, const int32_t *refs, float lox, float loy,
                          float loz, float cell, int nx, int ny, int nz, float guard, int cull_back, float *t,
                          int32_t *face, float *uv, int64_t *counters, sgnn_stream_t stream);
int sgnn_raytrace_occluded(const float *origins, const float *dirs, int64_t nrays, float t_min, const float *t_max,
                           const float *records, const int32_t *offsets, const int32_t *refs, float lox, float loy,
                           float loz, float cell, int nx, int ny, int nz, float guard, int cull_back, uint8_t *hit,
                           int64_t *counters, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Connected components of volumes and meshes (sgnn_amd.components; rules in INTEGRATION.md section J): lock-free
 * union-find on parent[] (i32, one slot per voxel or vertex; -1 = background / unreferenced).  Larger indices are
 * hooked onto smaller ones, so parent[i] <= i at all times and the root of a finished component is its smallest index.
 *   sgnn_cc_volume_link -> parent of a (nb, dz, dy, dx) u8 mask (non-zero = foreground), connectivity 6, 18 or 26 inside
 *                          one sample; nothing links across the batch axis or around a row end.  tiled != 0: every
 *                          SGNN_CC_TILE_Z x _Y x _X tile is labelled in LDS first and only pairs that straddle a tile
 *                          border are merged in global memory; tiled == 0: every pair is.  Both give the same
 *                          components.
 *   sgnn_cc_mesh_link   -> parent of nverts vertices: the three vertices of every face are joined.  A face with an
 *                          index outside [0, nverts) is skipped before any access and raises
 *                          SGNN_STATUS_COORD_RANGE in *status (status may be NULL).
 *   sgnn_cc_flatten     -> parent[i] = root of i; is_root[i] = (parent[i] == i), u8
 *   (caller: sel = sgnn_compact_mask(is_root), ncomp = its count; rank = sgnn_weld_number(sel): component k is the
 *    one with the k-th smallest minimum index)
 *   sgnn_cc_relabel     -> labels[i] = rank[parent[i]] or -1; sizes[k] (i64, zeroed by the caller) += members of k
 *   sgnn_cc_face_labels -> face_labels[t] = vertex_labels[faces[t][0]] (-1 for a face with a bad index);
 *                          face_sizes[k] (i64, zeroed by the caller) += faces of k
 * Sizes are integer atomics: the same input gives the same output.  nb * dz * dy * dx < 2^31, nverts < 2^31,
 * 3 * ntri < 2^31; a label outside [0, ncomp) is never used as an index.
 * ------------------------------------------------------------------------- */
#define SGNN_CC_TILE_Z 8
#define SGNN_CC_TILE_Y 8
#define SGNN_CC_TILE_X 32
int sgnn_cc_volume_link(const uint8_t *mask, int nb, int dz, int dy, int dx, int connectivity, int tiled,
                        int32_t *parent, sgnn_stream_t stream);
int sgnn_cc_mesh_link(const int32_t *faces, int ntri, int nverts, int32_t *parent, int32_t *status,
                      sgnn_stream_t stream);
int sgnn_cc_flatten(int32_t *parent, int64_t n, uint8_t *is_root, sgnn_stream_t stream);
int sgnn_cc_relabel(const int32_t *parent, int64_t n, const int32_t *rank, int64_t ncomp, int32_t *labels,
                    int64_t *sizes, sgnn_stream_t stream);
int sgnn_cc_face_labels(const int32_t *faces, int ntri, int nverts, const int32_t *vertex_labels, int64_t ncomp,
                        int32_t *face_labels, int64_t *face_sizes, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mesh simplification by vertex clustering with quadric placement (sgnn_amd.simplify; rules in INTEGRATION.md
 * section K).  The caller chains the stages and reads the counts back in between:
 *   sgnn_simp_keys     -> keys[i] = (cx << 42) | (cy << 21) | cz with c = floor((v - origin) / cell) in fp32 per axis;
 *                         origin: 3 floats on the device.  A non-finite coordinate or a cell index outside [0, 2^21)
 *                         gives the key -1 and raises SGNN_STATUS_COORD_RANGE in *status; such a vertex joins no cluster.
 *   sgnn_simp_clusters -> first_of[i] = smallest vertex index with vertex i's key (-1 for the key -1), is_first[i] u8;
 *                         tkeys (cap) i64 and tfirst (cap) i32 are the hash table, initialised here,
 *                         cap >= sgnn_weld_slots(nv)
 *   (caller: sel = sgnn_compact_mask(is_first), nclust = its count; rank = sgnn_weld_number(sel): cluster k is the
 *    one with the k-th smallest first member)
 *   sgnn_simp_corners  -> corner_first[3t + k] = first_of[faces[t][k]].  A face with an index outside [0, nverts) is
 *                         not dereferenced and raises SGNN_STATUS_COORD_RANGE in *status; it, and a face on a vertex
 *                         without a key, get vertex 0 three times: in range, and degenerate to every later stage.
 *   (caller: sgnn_mesh_faces(corner_first, rank) remaps the faces to cluster numbers and flags the ones that stay;
 *    sgnn_compact_mask + sgnn_take_rows3 -> kept faces)
 *   sgnn_simp_mark     -> used[c] = 1 (u8, zeroed by the caller) for every cluster c in [0, nclust) of cfaces (nfaces,3)
 *   (caller: csel = sgnn_compact_mask(used): output vertex p is cluster csel[p]; order = corner numbers sorted stably
 *    by cluster, start (nclust + 1) = where each cluster's corners begin in order)
 *   sgnn_simp_place    -> out_verts (nout,3) f32 and, with colors, out_colors (nout,3) u8 of the clusters csel[p]:
 *                         one lane per cluster sums its corners order[start[c] .. start[c+1]) in that order in fp64 and
 *                         solves for the vertex.  quadric = 1: section K's regularised quadric minimiser, 0: the mean.
 *                         sel[c] = first member of cluster c; keys as above.  A corner whose face has a bad index is
 *                         passed over.
 * No floating-point atomics anywhere: the same input gives the same bits.  nverts < 2^31, 3 * ntri < 2^31.
 * ------------------------------------------------------------------------- */
int sgnn_simp_keys(const float *verts, int64_t nv, const float *origin, float cell, int64_t *keys, int32_t *status,
                   sgnn_stream_t stream);
int sgnn_simp_clusters(const int64_t *keys, int64_t nv, int64_t *tkeys, int32_t *tfirst, int64_t cap,
                       int32_t *first_of, uint8_t *is_first, sgnn_stream_t stream);
int sgnn_simp_corners(const int32_t *faces, int ntri, int nverts, const int32_t *first_of, int32_t *corner_first,
                      int32_t *status, sgnn_stream_t stream);
int sgnn_simp_mark(const int32_t *cfaces, int64_t nfaces, int64_t nclust, uint8_t *used, sgnn_stream_t stream);
int sgnn_simp_place(const float *verts, int nverts, const int32_t *faces, int ntri, const uint8_t *colors,
                    const int64_t *order, const int64_t *start, const int32_t *csel, int64_t nout, const int32_t *sel,
                    const int64_t *keys, const float *origin, float cell, int quadric, float *out_verts,
                    uint8_t *out_colors, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mesh fairing (sgnn_amd.smooth; rules in INTEGRATION.md section Y).  Topology never changes: every stage reads faces
 * (ntri,3) i32 and rows of 3 floats and writes new rows.  A face with a repeated index contributes nothing anywhere; a
 * face with an index outside [0, nverts) is not dereferenced and raises SGNN_STATUS_COORD_RANGE in *status.
 * The adjacency, chained by the caller:
 *   sgnn_smooth_keys      -> keys (6 * ntri) i64: (a << 32 | b) for both directions of the three edges of every face,
 *                            2^63 - 1 six times for a face that contributes nothing
 *   (caller: sort the keys)
 *   sgnn_smooth_run_flags -> flags[j] u8 = 1 where sorted key j is a real key and differs from key j - 1
 *   (caller: sel = sgnn_compact_mask(flags), nruns = its count)
 *   sgnn_smooth_runs      -> source[r], neighbor[r] i32 = the two halves of the key of run r, mult[r] u8 = the length of
 *                            the run, clamped to 255: the number of faces on the undirected edge
 *   (caller: start (nverts + 1) i64 = exclusive scan of the counts of source)
 *   sgnn_smooth_classify  -> kind[i] u8: 0 no edge, 3 an edge of multiplicity above 2, else 2 an edge of multiplicity
 *                            1, else 1
 * One umbrella step:
 *   sgnn_smooth_step      -> xout = xin + f * (mean of the used neighbours - xin) for every vertex that moves, xin
 *                            elsewhere; rows of `stride` floats (3, or 4 on 16-byte boundaries with the fourth written
 *                            as 0); mode 0 'fixed', 1 'curve', 2 'free' for kind 2; fixed (nverts) u8 or NULL; status
 *                            non-NULL: a non-finite coordinate of xin raises SGNN_STATUS_COORD_RANGE.  xin != xout.
 * Normals.  order (3 * ntri) i64 is the stable sort of the corner keys by vertex and cstart (nverts + 2) i64 the
 * exclusive scan of their counts (list nverts holds the corners of the faces that contribute nothing):
 *   sgnn_smooth_face_normals   -> out (ntri,3): (b - a) x (c - a), divided by its length if unit (0 where that is 0);
 *                                 status may be NULL
 *   sgnn_smooth_corners        -> ckeys[3t + k] = faces[t][k], or nverts for a face that contributes nothing
 *   sgnn_smooth_vertex_normals -> out (nverts,3): the unit sum of raw (ntri,3) over the faces of every vertex's list
 * Denoising:
 *   sgnn_smooth_filter    -> nout (ntri,3): one pass of the face-normal filter over nin, nin != nout
 *   sgnn_smooth_update    -> xout (nverts,3): one pass of the vertex update towards the planes of the filtered
 *                            normals; kind, fixed and status as in sgnn_smooth_step
 * One lane per vertex or face sums its list in order; no floating-point atomics: the same input gives the same bits.
 * nverts < 2^31, 6 * ntri < 2^31.
 * ------------------------------------------------------------------------- */
int sgnn_smooth_keys(const int32_t *faces, int ntri, int nverts, int64_t *keys, int32_t *status, sgnn_stream_t stream);
int sgnn_smooth_run_flags(const int64_t *keys, int64_t n, uint8_t *flags, sgnn_stream_t stream);
int sgnn_smooth_runs(const int64_t *keys, int64_t n, const int32_t *sel, int64_t nruns, int32_t *source,
                     int32_t *neighbor, uint8_t *mult, sgnn_stream_t stream);
int sgnn_smooth_classify(const int64_t *start, const uint8_t *mult, int nverts, uint8_t *kind, sgnn_stream_t stream);
int sgnn_smooth_step(const float *xin, float *xout, int nverts, int stride, const int64_t *start,
                     const int32_t *neighbor, const uint8_t *mult, const uint8_t *kind, const uint8_t *fixed, int mode,
                     float f, int32_t *status, sgnn_stream_t stream);
int sgnn_smooth_face_normals(const float *verts, int nverts, const int32_t *faces, int ntri, int unit, float *out,
                             int32_t *status, sgnn_stream_t stream);
int sgnn_smooth_corners(const int32_t *faces, int ntri, int nverts, int32_t *ckeys, int32_t *status,
                        sgnn_stream_t stream);
int sgnn_smooth_vertex_normals(const float *raw, int ntri, const int64_t *order, const int64_t *cstart, int nverts,
                               float *out, sgnn_stream_t stream);
int sgnn_smooth_filter(const float *nin, float *nout, const int32_t *faces, int ntri, int nverts, const int64_t *order,
                       const int64_t *cstart, float threshold, sgnn_stream_t stream);
int sgnn_smooth_update(const float *xin, float *xout, int nverts, const int32_t *faces, int ntri, const float *normals,
                       const int64_t *order, const int64_t *cstart, const uint8_t *kind, const uint8_t *fixed,
                       int32_t *status, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Point-cloud neighbourhoods (sgnn_amd.cloud; rules in INTEGRATION.md section Z).  Points and queries are rows of 3
 * floats; a row with a non-finite coordinate is never a neighbour and gets the empty answer as a query.  The grid is
 * (lox, loy, loz, cell, nx, ny, nz): at most 1024 cells an axis and fewer than 2^31 - 1 in all, x fastest; the cell of
 * a coordinate is floor((p - lo) / cell) in fp32, clamped to the grid.  No answer depends on the grid.
 * The index, chained by the caller:
 *   sgnn_cloud_keys   -> keys[i] i64 = (cell << 32 | i), cell 2^31 - 1 for a non-finite row (points and queries alike)
 *   (caller: sort the keys; nfin = the number of finite rows)
 *   sgnn_cloud_pack   -> packed (nfin,4) f32 on a 16-byte boundary: (x, y, z, bits of the index) in key order, and
 *                        start (ncell + 1) i32: the first record of every cell
 * Queries.  qkeys are the sorted keys of the queries; queries == NULL takes the indexed points themselves as queries
 * (nq = nfin, qkeys unused), each without its own row, and writes to row `index` of nrows:
 *   sgnn_cloud_knn          -> idx (nrows,k) i32 and d2 (nrows,k) f32: the first k of (d2, index) with d2 <= limit2,
 *                              -1 and +inf where there are fewer; k in [1, 32]; d2 = (dx*dx + dy*dy) + dz*dz in fp32
 *   sgnn_cloud_radius_count -> count[q] i32 = the points with d2 <= limit2
 *   sgnn_cloud_radius_fill  -> out[qstart[q] + .] i64 = (q << 32 | index) of those points in no order, qstart
 *                              (nq + 1) i64 the exclusive scan of count (the caller sorts out)
 * Consumers of the rows of sgnn_cloud_knn over the points themselves:
 *   sgnn_cloud_normals   -> normal (n,3) f32, variation (n) f32, valid (n) u8 by fp64 covariance and five cyclic Jacobi
 *                           sweeps; toward_mode 0 none (toward NULL), 1 one viewpoint (3 floats), 2 one per point (n,3)
 *   sgnn_cloud_mean_dist -> mean (n) f64: the mean of the fp32 roots of the row, +inf for an empty row
 * Voxel down-sampling on the world lattice:
 *   sgnn_cloud_voxel_keys   -> keys[i] i64: 21 bits an axis (z, y, x from the top) of floor(p / cell) + 2^20 - 1, 2^63 - 1
 *                              for a non-finite row and for a cell at or beyond +-2^20, which also raises
 *                              SGNN_STATUS_COORD_RANGE in *status
 *   (caller: stable sort -> keys, order)
 *   sgnn_cloud_run_flags    -> flags[j] u8 = 1 where sorted key j is a real key and differs from key j - 1
 *   (caller: sel = sgnn_compact_mask(flags), nruns = its count, nvalid = the number of real keys)
 *   sgnn_cloud_voxel_reduce -> per run: mean position (fp64 sum in member order / count), rounded colour means (ncol 3
 *                              or 4, or 0 with colors NULL), unit sum of normals (or NULL), count, first member, and
 *                              cell_of[member] = run
 * No floating-point atomics: the same input gives the same bits.  Every count is below 2^31.
 * ------------------------------------------------------------------------- */
int sgnn_cloud_keys(const float *points, int64_t n, float lox, float loy, float loz, float cell, int nx, int ny, int nz,
                    int64_t *keys, sgnn_stream_t stream);
int sgnn_cloud_pack(const float *points, int64_t n, const int64_t *keys, int64_t nfin, int64_t ncell, float *packed,
                    int32_t *start, sgnn_stream_t stream);
int sgnn_cloud_knn(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy, float loz, float cell,
                   int nx, int ny, int nz, const float *queries, const int64_t *qkeys, int64_t nq, int64_t nrows, int k,
                   float limit2, int32_t *idx, float *d2, sgnn_stream_t stream);
int sgnn_cloud_radius_count(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy, float loz,
                            float cell, int nx, int ny, int nz, const float *queries, const int64_t *qkeys, int64_t nq,
                            float limit2, int32_t *count, sgnn_stream_t stream);
int sgnn_cloud_radius_fill(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy, float loz,
                           float cell, int nx, int ny, int nz, const float *queries, const int64_t *qkeys, int64_t nq,
                           float limit2, const int64_t *qstart, int64_t *out, sgnn_stream_t stream);
int sgnn_cloud_normals(const float *points, int64_t n, const int32_t *nbr, int k, const float *toward, int toward_mode,
                       float *normal, float *variation, uint8_t *valid, sgnn_stream_t stream);
int sgnn_cloud_mean_dist(const int32_t *nbr, const float *d2, int64_t n, int k, double *mean, sgnn_stream_t stream);
int sgnn_cloud_voxel_keys(const float *points, int64_t n, float cell, int64_t *keys, int32_t *status,
                          sgnn_stream_t stream);
int sgnn_cloud_run_flags(const int64_t *keys, int64_t n, uint8_t *flags, sgnn_stream_t stream);
int sgnn_cloud_voxel_reduce(const float *points, int64_t n, const uint8_t *colors, int ncol, const float *normals,
                            const int64_t *order, const int32_t *sel, int64_t nruns, int64_t nvalid, float *out_points,
                            uint8_t *out_colors, float *out_normals, int32_t *count, int32_t *first, int32_t *cell_of,
                            sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Triangle meshes to signed distance volumes (sgnn_amd.voxelize; rules in INTEGRATION.md section L).  The mesh is in
 * grid coordinates (voxel (i, j, k) has its centre at the integer point); records, boxes and usable come from
 * sgnn_meshdist_pack.  Volumes are (dz, dy, dx), x fastest, every dimension in [1, 65535] and fewer than 2^31 voxels;
 * band in [0, 65535] voxels.  Bricks are 8 x 8 x 8 voxels, brick (bx, by, bz) has the number (bz * nby + by) * nbx + bx
 * with nb = ceil(d / 8).  The caller chains the stages:
 *   sgnn_vox_grid_coords  -> out (nv,3) f32 = world2grid (host, 12 floats: rows 0..2 of the 4x4) applied to verts,
 *                            ((m0 x + m1 y) + m2 z) + m3 per row
 *   sgnn_vox_bricks_count -> counts[brick] += faces whose dilated box touches the brick (the caller zeroes counts)
 *   (caller: offsets = exclusive scan of counts; bricks = sgnn_compact_mask(counts > 0))
 *   sgnn_vox_bricks_fill  -> refs[offsets[brick] + k] = face, k from the zeroed cursor array; order inside a list is
 *                            not defined and does not matter
 *   sgnn_vox_normals      -> the pseudo-normal sums of rule 5 in 2^-32 fixed point: vsum (nverts,3) i64 per vertex,
 *                            esum (cap,3) i64 per slot of the edge table ekeys (cap) i64 / efirst (cap) i32, all
 *                            initialised here; cap >= sgnn_weld_slots(3 * ntri)
 *   sgnn_vox_nearest      -> dist f32 (signed, in voxels) and face i32 of every voxel of the nbricks listed bricks:
 *                            one workgroup per brick, face records staged through LDS SGNN_VOX_BATCH at a time.  Voxels
 *                            beyond the band get +inf and -1; voxels of other bricks are not written (the caller fills
 *                            them with +inf and -1 beforehand).  flip != 0 negates the pseudo-normals.
 *   sgnn_vox_tsdf         -> sdf[i] = dist[i] * voxel_size where face[i] >= 0, -inf elsewhere; weight[i] u8 = 1 / 0
 * Integer atomics only: the same input gives the same bits.
 * ------------------------------------------------------------------------- */
#define SGNN_VOX_BATCH 128
int sgnn_vox_grid_coords(const float *verts, int64_t nv, const float *world2grid, float *out, sgnn_stream_t stream);
int sgnn_vox_bricks_count(const float *boxes, int ntri, float band, int dx, int dy, int dz, int32_t *counts,
                          sgnn_stream_t stream);
int sgnn_vox_bricks_fill(const float *boxes, int ntri, float band, int dx, int dy, int dz, const int32_t *offsets,
                         int32_t *cursor, int32_t *refs, sgnn_stream_t stream);
int sgnn_vox_normals(const float *records, const int32_t *faces, const uint8_t *usable, int ntri, int nverts,
                     int64_t *vsum, int64_t *ekeys, int32_t *efirst, int64_t *esum, int64_t cap, sgnn_stream_t stream);
int sgnn_vox_nearest(const float *records, const float *boxes, const int32_t *faces, const int32_t *offsets,
                     const int32_t *refs, const int32_t *bricks, int nbricks, int dx, int dy, int dz, float band,
                     int flip, const int64_t *vsum, const int64_t *ekeys, const int64_t *esum, int64_t cap, float *dist,
                     int32_t *face, sgnn_stream_t stream);
int sgnn_vox_tsdf(const float *dist, const int32_t *face, int64_t n, float voxel_size, float *sdf, uint8_t *weight,
                  sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Euclidean feature transform of a dense seed mask (sgnn_amd.edt; rules in INTEGRATION.md section O): for every voxel
 * of a (dz, dy, dx) volume, x fastest, the nearest seed and the squared distance to it, exactly, in integers.  Among
 * seeds at the same squared distance the one with the smallest linear index (sz * dy + sy) * dx + sx wins.  Every
 * dimension is at most SGNN_EDT_MAX_DIM and there are fewer than 2^31 voxels; a volume without voxels is a no-op.
 * max_dist2 < 0: no cap; otherwise a voxel whose nearest seed is farther than max_dist2 (squared, in voxels) has none,
 * and every other voxel gets what it gets without a cap.  The caller chains three passes:
 *   sgnn_edt_rows -> feat[p] = the nearest seed of p inside p's row, equal distances to the smaller x, packed as
 *                    sz << 20 | sy << 10 | sx, or -1 (mask: u8, non-zero = seed)
 *   sgnn_edt_axis -> one pass along y (axis 1) or z (axis 0) over the features of the pass before: the candidate of
 *                    p = the feature of a voxel of p's column that is nearest to p, equal distances to the smaller
 *                    packed value.  With dist2 and nearest NULL it writes packed features to feat_out; with both
 *                    given it is the last pass and writes dist2 (i32) and nearest (i32 linear index), -1 / -1 for
 *                    none, and feat_out is not used.  No output may be feat_in.
 * x, then y, then z gives the rule above (the lexicographically smallest (sz, sy, sx) among the nearest).
 *   sgnn_edt_fill -> out[p] = colors[nearest[p]] (3 bytes) where nearest[p] is in [0, n), else 0; out is not colors
 * Integer arithmetic only and no atomics: the same input gives the same output.
 * ------------------------------------------------------------------------- */
#define SGNN_EDT_MAX_DIM 1024
int sgnn_edt_rows(const uint8_t *mask, int dz, int dy, int dx, int max_dist2, int32_t *feat, sgnn_stream_t stream);
int sgnn_edt_axis(const int32_t *feat_in, int dz, int dy, int dx, int axis, int max_dist2, int32_t *feat_out,
                  int32_t *dist2, int32_t *nearest, sgnn_stream_t stream);
int sgnn_edt_fill(const uint8_t *colors, const int32_t *nearest, int64_t n, uint8_t *out, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Point clouds with known sensor origins fused into a scan volume (sgnn_amd.points; rules in INTEGRATION.md
 * section P).  The volume is the (sdf, weight, free_ctr[, color]) state of the fusion block above.  points (nrays, 3)
 * and origins (norigins, 3) f32 world metres; origin_id (nrays) i32 or NULL (all 0); world2grid / grid2world: host
 * float[12], rows 0..2 of the fp32 matrices; obb: host float[12] as in sgnn_fuse_integrate, or NULL.  One call of
 * points.integrate chains:
 *   sgnn_points_count -> counts[r] = the number of half-voxel samples of ray r (0: the ray is ignored, or its segment
 *                        cannot touch the grid); box (device int32[8]) = x0, x1, y0, y1, z0, z1, inclusive, of the
 *                        voxels the call's segments can touch (x0 > x1: none), box[6] = 1 if an origin id is outside
 *                        [0, norigins) (such rays are ignored), box[7] = 0
 *   (offsets = exclusive scan of counts, nrays + 1 int64, made by the caller)
 *   sgnn_points_walk  -> one lane per sample; integer atomic adds into accumulators that cover the box only (host
 *                        int32[6], read back from sgnn_points_count), x fastest: acc_s int64 = sum q wi,
 *                        acc_wf u64 = free count << 32 | sum wi, acc_c 4 u64 per voxel = sum R wi, G wi, B wi, wi
 *                        (NULL iff colors (nrays, channels = 3 | 4) u8 is NULL).  The accumulators are zero before
 *                        the first walk of a call; several walks over parts of the rays add up.  max_samples: the
 *                        caller's upper bound on offsets[nrays], which only sizes the launch.
 *   sgnn_points_fold  -> the accumulators folded into the volume as ONE observation per voxel
 * Integer atomics only: the same rays in any order, in any split, give the same bits.
 * ------------------------------------------------------------------------- */
#define SGNN_POINTS_MAX_RAYS (1ll << 28)
int sgnn_points_count(const float *points, const float *origins, const int32_t *origin_id, int64_t nrays, int norigins,
                      const float *world2grid, int dx, int dy, int dz, float voxel_size, float depth_min,
                      float depth_max, int carve, int32_t *counts, int32_t *box, sgnn_stream_t stream);
int sgnn_points_walk(const float *points, const float *origins, const int32_t *origin_id, const uint8_t *colors,
                     int channels, int64_t nrays, int norigins, const int64_t *offsets, int64_t max_samples,
                     const float *world2grid, const float *grid2world, const float *obb, int dx, int dy, int dz,
                     float voxel_size, float depth_min, float depth_max, int carve, const int32_t *box, int64_t *acc_s,
                     uint64_t *acc_wf, uint64_t *acc_c, sgnn_stream_t stream);
int sgnn_points_fold(float *sdf, uint8_t *weight, int32_t *free_ctr, uint16_t *color, int dx, int dy, int dz,
                     float voxel_size, const int32_t *box, const int64_t *acc_s, const uint64_t *acc_wf,
                     const uint64_t *acc_c, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * A TSDF volume's state moved to another grid (sgnn_amd.regrid; rules in INTEGRATION.md section Q).  Both volumes are
 * the (sdf, weight, free_ctr[, color]) state of the fusion block above, (dz, dy, dx) with x fastest.  map: host
 * float[12], rows 0..2 of A = src.world2grid . inv(dst.world2grid), which takes a destination voxel to source voxel
 * coordinates.  linear: 1 = rule Q.5, 0 = rule Q.4 (nearest).  skip: 1 = a block whose destination box provably misses
 * the source grid takes the short path; the result never depends on it.  shape: the destination brick of a wave,
 * 0 = 4 x 4 x 4, 1 = 8 x 8 x 1, 2 = 64 x 1 x 1; the result never depends on it.
 *   sgnn_regrid_resample -> every destination voxel is written; color pointers both NULL or both set
 *   sgnn_regrid_merge    -> the resampled state is folded into the destination (rule Q.8); colour is folded only
 *                           where both pointers are set
 * The two volumes must not share memory.
 * ------------------------------------------------------------------------- */
int sgnn_regrid_resample(const float *src_sdf, const uint8_t *src_weight, const int32_t *src_free,
                         const uint16_t *src_color, int sdx, int sdy, int sdz, const float *map, int linear, int skip,
                         int shape, float *dst_sdf, uint8_t *dst_weight, int32_t *dst_free, uint16_t *dst_color,
                         int ddx, int ddy, int ddz, sgnn_stream_t stream);
int sgnn_regrid_merge(const float *src_sdf, const uint8_t *src_weight, const int32_t *src_free,
                      const uint16_t *src_color, int sdx, int sdy, int sdz, const float *map, int linear, int skip,
                      int shape, float *dst_sdf, uint8_t *dst_weight, int32_t *dst_free, uint16_t *dst_color, int ddx,
                      int ddy, int ddz, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Evaluation metrics on the device.
 * ------------------------------------------------------------------------- */
/* IoU ingredients of one hierarchy level (torch/loss.py:84-120 compute_iou_sparse_dense, fed as in
 * torch/train.py:271-290).  Rows r of locs (m,4 int64 z,y,x,b) count when keep[r] != 0, or — keep == NULL —
 * when sigmoid(logits[r*lstride]) > 0.5, or always when both are NULL.  tgt: dense (nb,1,d0,d1,d2) occupancy,
 * float {0,1,-1 = unknown} or uint8 {0,1,255} (the reference's `.byte()` of -1).  counters (device int64
 * [nb][3]) receive per sample {P = counted rows (minus rows on unknown voxels if use_mask), C = those whose
 * target is 1, T = voxels with target 1}: intersection = C, union = P + T - C. */
int sgnn_iou_counts(const int64_t *locs, const uint8_t *keep, const float *logits, int64_t lstride, int64_t m,
                    const void *tgt, int tgt_is_u8, int nb, int d0, int d1, int d2, int use_mask,
                    int64_t *counters, sgnn_stream_t stream);
/* mean |pred - target| over target-surface voxels (torch/loss.py:201-231 compute_l1_tgtsurf_sparse_dense):
 * surface = |t| < truncation (thresh < 0) or |t| <= thresh; voxels without a prediction count as -truncation;
 * known != NULL drops voxels with known >= 2.  out3 (device double[3]) = {sum, count, mean}. */
int64_t sgnn_l1_tgtsurf_ws_bytes(void);
int sgnn_l1_tgtsurf(const int64_t *locs, const float *vals, int64_t m, const float *tgt_sdf, const uint8_t *known,
                    int nb, int d0, int d1, int d2, float truncation, float thresh, double *out3, void *ws,
                    int64_t ws_bytes, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Marching cubes + mesh clean-up on the device.  Replaces
 * torch/marching_cubes/marching_cubes.cpp: run_marching_cubes_internal (:458-476), merge_close_vertices with
 * approx = true (:359-456), remove_degenerate_faces (:298-321), remove_duplicate_faces (:266-297) — same vertex
 * order, same indices, same bits.  The caller chains the stages and reads the counts back in between:
 *   sgnn_mc_count  -> *ntri (device)          triangles the volume produces; keeps per-voxel counts in ws
 *   sgnn_mc_emit   -> verts (3*ntri,3) f32 x,y,z and vcols (3*ntri,3) u8, in the reference's z,y,x voxel order
 *   sgnn_weld_build / sgnn_weld_sweep (repeat until *undecided == 0) / sgnn_weld_lookup
 *                  -> creator_of[i] = the soup vertex that vertex i is merged into, is_creator[i]
 *   sgnn_compact_mask(is_creator) -> sel;  sgnn_weld_number(sel) -> newid;  sgnn_take_rows3 -> welded verts / colours
 *   sgnn_mesh_faces -> faces (ntri,3) remapped + keep[t] (not degenerate, first of its vertex triple);
 *   sgnn_compact_mask(keep) + sgnn_take_rows3 -> final faces.
 * tsdf: dense (d0,d1,d2) = (z,y,x) f32, -inf or |d| >= truncation = no data; colors: (d0,d1,d2,3) u8 or NULL (220).
 * ------------------------------------------------------------------------- */
int64_t sgnn_mc_ws_bytes(int d0, int d1, int d2);
int sgnn_mc_count(const float *tsdf, int d0, int d1, int d2, float isovalue, float truncation, float thresh,
                  void *ws, int64_t ws_bytes, int64_t *ntri, sgnn_stream_t stream);
int sgnn_mc_emit(const float *tsdf, const uint8_t *colors, int d0, int d1, int d2, float isovalue,
                 float truncation, float thresh, void *ws, int64_t ws_bytes, float *verts, uint8_t *vcols,
                 sgnn_stream_t stream);
/* cells (nv,3) i32 = grid cell of every vertex at pitch `thresh` (the reference passes 1e-5);
 * rep/first (cap) i32, state (cap) u8: the cell table, initialised here */
int sgnn_weld_build(const float *verts, int64_t nv, float thresh, int32_t *cells, int32_t *rep, int32_t *first,
                    uint8_t *state, int64_t cap, sgnn_stream_t stream);
/* one sweep of the creation fixed point; *undecided (device) = cells still open after it */
int sgnn_weld_sweep(const int32_t *cells, const int32_t *rep, const int32_t *first, uint8_t *state, int64_t cap,
                    int64_t *undecided, sgnn_stream_t stream);
int sgnn_weld_lookup(const int32_t *cells, int64_t nv, const int32_t *rep, const int32_t *first,
                     const uint8_t *state, int64_t cap, int32_t *creator_of, uint8_t *is_creator,
                     sgnn_stream_t stream);

/* Shared mesh tables (csrc/mesh_tables.hip): what marching cubes' clean-up, sgnn_amd.components and sgnn_amd.simplify
 * have in common. */
/* hash slots needed for n keys (vertices for the weld and the clusters, triangles for the duplicate-face set) */
int64_t sgnn_weld_slots(int64_t n);
/* newid[sel[p]] = p */
int sgnn_weld_number(const int32_t *sel, int64_t n, int32_t *newid, sgnn_stream_t stream);
int sgnn_mesh_faces(const int32_t *creator_of, const int32_t *newid, int64_t ntri, int32_t *faces, int32_t *frep,
                    int32_t *ffirst, int64_t cap, uint8_t *keep, sgnn_stream_t stream);
/* dst row p = src row sel[p] for (.,3) arrays of 1- or 4-byte elements */
int sgnn_take_rows3(const void *src, int elem_bytes, const int32_t *sel, int64_t n, void *dst, sgnn_stream_t stream);

/* ---------------------------------------------------------------------------
 * Optional live timing of the convolution launches (bench.py's roofline leg): HIP events are
 * recorded on the caller's stream around every sgnn_conv_fwd (kind 0) / sgnn_conv_bwd_weight
 * main kernel (kind 1).  Off by default.  sgnn_prof_get must follow a stream synchronise.
 * ------------------------------------------------------------------------- */
int sgnn_prof_enable(int max_records);
int sgnn_prof_disable(void);
int sgnn_prof_resume(void); /* keep the records gathered so far */
int sgnn_prof_count(void);
int sgnn_prof_dropped(void);
/* kernel launches issued by this library so far in this process (difference around a step = its launches) */
int64_t sgnn_launch_count(void);
int sgnn_prof_get(int i, int *kind, int64_t *n_out, int *cin, int *cout, int *K, int *flags, float *ms);

/* Device time stamps inside a captured graph (measurement only; scripts/lane_stamps.py).  sgnn_stamp launches a one-thread
 * kernel that writes the device's constant 100 MHz clock into the next slot of `buf` and remembers `label` for it; while no
 * buffer is enabled it launches nothing and returns -1.  Slots are handed out in call order since the last
 * sgnn_stamp_reset / _enable, so a captured step re-writes the same slots on every replay.  buf: max_stamps int64 on
 * the device (NULL, 0 switches stamps off).  SGNN_STAMP_ONLY=label,label,... in the environment keeps only those labels
 * (a stamp is a graph node, and WHERE a node sits decides which stream the HIP graph executor gives its successors:
 * profiles/r06y_graph_executor.txt). */
int sgnn_stamp_enable(int64_t *buf, int max_stamps);
int sgnn_stamp_reset(void);
int sgnn_stamp(const char *label, sgnn_stream_t stream);
int sgnn_stamp_count(void);
const char *sgnn_stamp_label(int i);

#ifdef __cplusplus
}
#endif
#endif /* SGNN_HIP_H */
