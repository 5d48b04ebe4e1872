// Sparse-network program executor: runs a whole static sub-network — an encoder level stack, or a complete
// generative stage (skip join -> SubmanifoldConvolution -> FullyConvolutionalNet U -> BatchNormReLU -> 8-child
// up-sampling convolution -> BatchNormReLU -> the two linear heads) — forward or backward from ONE call.
//
// Counterpart of what upstream does with Python nn.Module containers (scn.Sequential / ConcatTable / AddTable /
// JoinTable composing <Op>_updateOutput calls): the reference's model.py builds those containers at
// torch/model.py:31-47, 178-191, 253-258 and glues them with tensor ops at :209-247, 259-272, 338-355; here the tree
// is compiled once into a flat op list (sgnn_amd/scn/program.py) and interpreted natively.  A training step is
// host-bound (every microsecond of host time shows up in the step time, profiles/r02_host_bound.txt): one native call
// per stage and direction replaces ~12 Python autograd nodes and their tensor allocations.
// Host-side code only: no kernels here.
#include <mutex>
#include <vector>
#include "common.h"
#include "bn_fuse.h"

enum {
  OP_CONV_SUBM = 0, OP_CONV_DOWN = 1, OP_UNPOOL = 2, OP_BN = 3, OP_ADD = 4, OP_JOIN = 5,
  OP_CONCAT_IN = 6,   // out = [in0[ia] | in1[ib] | in2[ic]]  (index arrays optional; inputs may be externals)
  OP_EXPAND = 7,      // SubmanifoldConvolution over the 8-child expansion, on the parent rulebook (sgnn_conv_fwd_ex)
  OP_LINEAR = 8       // cout (1 or 2) per-site heads; weight row o = param slot par + 2*o, its bias par + 2*o + 1
};
#define OPW 12   // ints per op: type, in0, in1, out, par, lev, cin, cout, in2, ia, ib, ic
#define EXPAND_DX_SPLIT 4

// conv.hip entry points without a prototype in the public header
extern "C" int sgnn_expand_weights(const float *w, int cin, int cout, float *wc, sgnn_stream_t stream);
extern "C" int sgnn_expand_weights_bwd(const float *dwc, int cin, int cout, float *dw, sgnn_stream_t stream);
// infer_bf16.hip: the kernels of the bf16 inference layout
int64_t sgnn_bf16_wfrag_bytes(int cin, int cout, int K, int groups);
int sgnn_bf16_conv_prepare(const float *w, int cin, int cout, int K, int groups, void *wf, sgnn_stream_t stream);
int sgnn_bf16_conv_run(const void *x, int64_t n_in, int cin, int64_t ldx, const float *w, const void *wf, int K,
                       const int32_t *table, int64_t ld, int64_t n_out, int cout, void *y, int64_t ldy,
                       const void *addend, int64_t ld_add, const int32_t *kmap, int groups, int table_rows,
                       const int64_t *n_dev, sgnn_stream_t stream);
int sgnn_bf16_conv_expand_impl(const void *x, int64_t n, int cin, int64_t ldx, const float *w, const int32_t *nbr,
                               int64_t ld, int cout, void *y, int64_t ldy, const int64_t *n_dev, void *ws,
                               sgnn_stream_t stream);
int sgnn_bf16_linear_rows(const void *x, int64_t ldx, int64_t n, int cin, const float *const *w, const float *const *b,
                          int cout, float *y, const int64_t *n_dev, sgnn_stream_t stream);

namespace {

// One record of the caller's op array (sgnn_amd/scn/program.py writes it), field for field
struct Op {
  int32_t type, in0, in1, out, par, lev, cin, cout, in2, ia, ib, ic;
  bool is_conv() const { return type == OP_CONV_SUBM || type == OP_CONV_DOWN; }
  int K() const { return type == OP_CONV_DOWN ? 8 : 27; }                    // kernel offsets of the weight tensor
  int out_class() const { return type == OP_CONV_DOWN ? lev + 1 : lev; }     // rows class of the output
  template <class F>
  void for_inputs(F f) const {   // every buffer the op reads (-1: an optional input that is absent)
    f(in0);
    if (type == OP_ADD || type == OP_JOIN || type == OP_CONCAT_IN) f(in1);
    if (type == OP_CONCAT_IN) f(in2);
  }
};
static_assert(sizeof(Op) == sizeof(int32_t[OPW]), "Op mirrors one record of the caller's int32 array");

struct View {
  const int32_t *ops;   // nops x OPW
  const float *opf;     // nops x 4: eps, momentum, leak, unused
  int nops;
  const int32_t *bufs;  // nbuf x 2: rows class ("level"), channels
  int nbuf, n_ext;      // buffers [0, n_ext) are caller-owned inputs outside the arena
  const int64_t *lev_n, *lev_ld;
  void *const *lev_nbr, *const *lev_children, *const *lev_ptable, *const *lev_parent;
  int nlev;
  const Op &op(int i) const { return reinterpret_cast<const Op *>(ops)[i]; }
};

// Which arena layout a call uses: every buffer keeps its storage (a backward call reads the arena), liveness-packed
// (make_layout_infer), or that with bf16 storage (eval only).  The entry points spell it three ways (`mode`, `infer`, the
// bits of `training`); each decodes its spelling into this where it enters.
enum Kind { TRAINING, INFERENCE, INFERENCE_BF16 };

// `mode` 0..3 of sgnn_prog_arena_floats / sgnn_prog_plan (0 and 1 differ in what is reported, not in the layout)
Kind kind_of_mode(int mode) { return mode == 3 ? INFERENCE_BF16 : mode == 2 ? INFERENCE : TRAINING; }

inline int64_t round64(int64_t v) { return (v + 63) & ~int64_t(63); }

// What a convolution op (OP_CONV_SUBM, OP_CONV_DOWN) launches with, forward and backward.  The sizing entry points
// pass no tables: the rows alone are filled in then.
struct ConvSetup {
  bool ok = false;                                   // the levels it names exist (a stride-2 op needs level lev + 1)
  int K = 0, cnt_class = 0;                          // cnt_class: rows class whose device count bounds the output
  int64_t n = 0, n_out = 0;                          // rows of the input (level lev); rows of the output = rows of dy
  const int32_t *tab_f = nullptr, *tab_b = nullptr;  // forward table (also the weight gradient's), data-gradient table
  int64_t ld_f = 0, ld_b = 0;                        // their lds
  int flags_b = 0;                                   // flags of the data-gradient launch
  ConvSetup(const View &v, const Op &o) {
    const bool down = o.type == OP_CONV_DOWN;
    K = o.K();
    cnt_class = o.out_class();
    ok = o.lev >= 0 && cnt_class < v.nlev;
    if (!ok) return;
    n = v.lev_n[o.lev];
    n_out = v.lev_n[cnt_class];
    if (!v.lev_ld) return;
    tab_f = (const int32_t *)(down ? v.lev_children[o.lev] : v.lev_nbr[o.lev]);
    ld_f = v.lev_ld[cnt_class];
    tab_b = (const int32_t *)(down ? v.lev_ptable[o.lev] : v.lev_nbr[o.lev]);
    ld_b = v.lev_ld[o.lev];
    flags_b = down ? SGNN_CONV_TRANSPOSE_W : (SGNN_CONV_TRANSPOSE_W | SGNN_CONV_FLIP_K);
  }
};

// number of ops that read buffer b
std::vector<int> count_readers(const View &v) {
  std::vector<int> r(v.nbuf, 0);
  for (int i = 0; i < v.nops; ++i)
    v.op(i).for_inputs([&](int b) {
      if (b >= 0 && b < v.nbuf) ++r[b];
    });
  return r;
}

// (the executor's switches live in the library's one table, sgnn_tune: prog_fusion, prog_lin_add, prog_lin_bn — tune.hip)
#define g_fuse (g_tune.prog_fusion != 0)
#define g_lin_add (g_tune.prog_lin_add != 0)
#define g_lin_bn (g_tune.prog_lin_bn != 0)
#define g_bn_fold (g_tune.prog_bn_fold_small != 0)
// What the executor decides once per call, identically in forward and backward:
//  * add_dst[i] >= 0: convolution i writes straight into the output of the AddTable right behind it (fused add);
//  * views: a JoinTable whose inputs can be produced in place gets no copy — its inputs LIVE in column ranges of the
//    join buffer (root / col / ld), every producer writes and every consumer reads through a row stride;
//  * fold[i] >= 0: BatchNormReLU i launches nothing — convolution fold[i], its only reader, applies it to the rows it
//    gathers (forward and weight gradient; pre_bn[fold[i]] = i).  Small levels of the training layout only (plan_bn_folds).
struct Plan {
  std::vector<int> add_dst;      // per op
  std::vector<int> add_src;      // per op: the other input of that AddTable, which the convolution adds while it stores
  std::vector<char> skip;        // per op: forward launches nothing (fused AddTable, in-place JoinTable)
  std::vector<int> root, col;    // per buffer: storage owner and column offset inside it
  std::vector<int64_t> ld;       // per buffer: row stride in floats
  std::vector<char> join_view;   // per op: this JoinTable is in place
  std::vector<int> fold, pre_bn; // per op: BatchNorm -> the convolution that applies it; convolution -> the BatchNorm it applies (-1: none)
  std::vector<int> lin_bn;       // per op: a LINEAR head whose data gradient is formed inside the backward pass of BatchNorm lin_bn[i] (BnLin; -1: written)
  Kind kind = TRAINING;          // INFERENCE_BF16: ld in bf16 elements, a multiple of 8 (LINEAR outputs: fp32, ld = channels)
  std::vector<char> f32;         // per buffer: stored as fp32 (always, except in the bf16 layout where only LINEAR outputs are)
  bool bf16() const { return kind == INFERENCE_BF16; }
};

inline int64_t round8(int64_t v) { return (v + 7) & ~int64_t(7); }

// this convolution shape can write its output and read its input (forward and data gradient) and form its weight
// gradient through a row stride
bool strided_conv_ok(const Op &o) {
  return sgnn_conv_epi_supported(o.cin, o.cout) && sgnn_conv_epi_supported(o.cout, o.cin) && dw_shape_ok(o.cin, o.cout);
}

// The convolution whose epilogue leaves the statistics partials of BatchNorm i in a training-mode forward pass (the
// convolution right in front of it, or in front of the AddTable fused into it), -1: the BatchNorm runs its own statistics pass
int stats_producer(const View &v, const Plan &P, int i) {
  const Op &b = v.op(i);
  for (int p = i - 1; p >= 0 && p >= i - 2; --p) {
    const Op &o = v.op(p);
    const bool fused_add = P.add_dst[p] >= 0;
    if (p + 1 + (fused_add ? 1 : 0) != i || !o.is_conv()) continue;
    if ((fused_add ? P.add_dst[p] : o.out) != b.in0) continue;
    if (!sgnn_conv_epi_supported(o.cin, o.cout) || ConvSetup(v, o).n_out <= 0) continue;
    return p;
  }
  return -1;
}

// BatchNorm i and the op right behind it have the shape of a fold (what can be told from the ops and the row counts alone)
bool fold_candidate(const View &v, int i) {
  if (i + 1 >= v.nops) return false;
  const Op &b = v.op(i), &o = v.op(i + 1);
  if (b.type != OP_BN || !o.is_conv() || o.in0 != b.out || o.lev != b.lev || o.cin != b.cin) return false;
  const ConvSetup cs(v, o);
  return cs.ok && sgnn_conv_fold_small_ok(o.cin, o.cout, cs.K, cs.n_out);
}

// BatchNormReLU folded into its only reader (sgnn_tune.prog_bn_fold_small).  On a small level the layer is one node of the
// dependent chain — arguments, two rounds over the partial table, two barriers, rows in, rows out — whose output is gathered
// once by the forward convolution and once by its weight gradient.  Folded, the convolution sums the table under its own rule
// and gather loads and the node disappears.  Only where
//  * the training layout is planned (the liveness-packed inference arenas keep the layer as a pass);
//  * nothing but ONE convolution reads the output (no AddTable, JoinTable, head or caller), the output is no view, that
//    convolution is the NEXT op (the layer's partial table lives in the shared statistics workspace: unfolded it is consumed
//    right behind its producer, and folded it must be too, before another convolution's epilogue writes there), and it runs
//    k_conv_small forward and k_conv_dw<.., 1> for its weight gradient (sgnn_conv_fold_small_ok);
//  * the statistics partials come from a convolution epilogue and pass bn_fuse_ok with the CONSUMER's grid, and
//    sgnn_tune.bn_fuse is on (the pass then sums the table in the same order: bit-identical statistics).
// The same decision in training and eval mode (eval reads the running statistics; no table), forward and backward.
// The backward pass needs no other change: k_bn_bwd_apply re-derives the ReLU mask from the BatchNorm input, the data
// gradient reads dy, and the only other reader of the output — the weight gradient — applies the layer itself.
void plan_bn_folds(const View &v, const std::vector<int> &readers, Plan &P) {
  if (!g_bn_fold || !g_tune.bn_fuse || P.kind != TRAINING) return;
  for (int i = 0; i < v.nops; ++i) {
    const Op &b = v.op(i);
    if (b.type != OP_BN || b.out < v.n_ext || b.out >= v.nbuf || readers[b.out] != 1 || P.root[b.out] != b.out) continue;
    if (b.lev < 0 || b.lev >= v.nlev || v.lev_n[b.lev] <= 0) continue;
    const int j = i + 1;
    if (j >= v.nops || !fold_candidate(v, i)) continue;
    const Op &o = v.op(j);
    const ConvSetup cs(v, o);
    if (!cs.ok || !sgnn_conv_fold_small_ok(o.cin, o.cout, cs.K, cs.n_out)) continue;
    const int p = stats_producer(v, P, i);
    if (p < 0) continue;
    const Op &po = v.op(p);
    const int64_t nblk = sgnn_conv_grid_blocks(ConvSetup(v, po).n_out, po.cin, po.cout, po.K());
    if (!bn_fuse_ok(nblk, b.cin, (cs.n_out + 15) / 16)) continue;
    P.fold[i] = j;
    P.pre_bn[j] = i;
  }
}

void make_plan(const View &v, const int32_t *keep, Plan &P, Kind kind) {
  P.kind = kind;
  P.f32.assign(v.nbuf, P.bf16() ? 0 : 1);
  if (P.bf16())
    for (int i = 0; i < v.nops; ++i)
      if (v.op(i).type == OP_LINEAR && v.op(i).out >= 0 && v.op(i).out < v.nbuf) P.f32[v.op(i).out] = 1;
  auto row_ld = [&](int r) -> int64_t { return P.f32[r] ? v.bufs[2 * r + 1] : round8(v.bufs[2 * r + 1]); };
  P.add_dst.assign(v.nops, -1);
  P.add_src.assign(v.nops, -1);
  P.skip.assign(v.nops, 0);
  P.join_view.assign(v.nops, 0);
  P.lin_bn.assign(v.nops, -1);
  P.fold.assign(v.nops, -1);
  P.pre_bn.assign(v.nops, -1);
  P.root.resize(v.nbuf);
  P.col.assign(v.nbuf, 0);
  P.ld.resize(v.nbuf);
  for (int b = 0; b < v.nbuf; ++b) {
    P.root[b] = b;
    P.ld[b] = row_ld(b);
  }
  if (!g_fuse) return;
  std::vector<int> readers = count_readers(v);
  if (keep)
    for (int b = 0; b < v.nbuf; ++b)
      if (keep[b]) ++readers[b];
  // a per-site head that is the ONLY reader of a BatchNormReLU's output: its data gradient is never stored (BnLin)
  if (g_lin_bn)
    for (int i = 0; i < v.nops; ++i) {
      const Op &o = v.op(i);
      if (o.type != OP_LINEAR || o.cout > 2 || readers[o.in0] != 1) continue;
      for (int j = 0; j < i; ++j) {
        const Op &b = v.op(j);
        if (b.type == OP_BN && b.out == o.in0 && b.lev == o.lev) P.lin_bn[i] = j;
      }
    }
  // fused AddTable
  for (int i = 0; i + 1 < v.nops; ++i) {
    const Op &o = v.op(i), &a = v.op(i + 1);
    if (!o.is_conv() || a.type != OP_ADD) continue;
    if (!sgnn_conv_epi_supported(o.cin, o.cout) || ConvSetup(v, o).n_out <= 0 || readers[o.out] != 1) continue;
    if ((a.in0 != o.out && a.in1 != o.out) || a.in0 == a.in1) continue;
    P.add_dst[i] = a.out;
    P.add_src[i] = a.in0 == o.out ? a.in1 : a.in0;
    P.skip[i + 1] = 1;
  }
  // producer op of every buffer (the fused convolution for a fused AddTable output) and its last reader
  std::vector<int> prod(v.nbuf, -1), last_reader(v.nbuf, -1);
  std::vector<char> strided_ok(v.nbuf, 1);   // every reader / writer of the buffer can work through a row stride
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    if (!P.skip[i]) prod[P.add_dst[i] >= 0 ? P.add_dst[i] : o.out] = i;
    auto reads = [&](int b, bool ok) {
      if (b < 0) return;
      last_reader[b] = i;
      if (!ok) strided_ok[b] = 0;
    };
    auto join_read = [&](int b) { return last_reader[b] >= 0 && v.op(last_reader[b]).type == OP_JOIN; };
    switch (o.type) {
      case OP_CONV_SUBM:
      case OP_CONV_DOWN: reads(o.in0, strided_conv_ok(o)); break;
      case OP_BN:
      case OP_UNPOOL: reads(o.in0, true); break;
      case OP_JOIN:
        reads(o.in0, !join_read(o.in0));   // two JoinTables reading it: no view
        reads(o.in1, !join_read(o.in1));
        break;
      case OP_ADD: reads(o.in0, P.skip[i] != 0); reads(o.in1, P.skip[i] != 0); break;   // a fused AddTable reads through the conv epilogue
      default: o.for_inputs([&](int b) { reads(b, false); }); break;
    }
  }
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    if (o.type != OP_JOIN || v.lev_n[o.lev] <= 0) continue;
    bool ok = true;
    for (int side = 0; side < 2 && ok; ++side) {
      const int q = side ? o.in1 : o.in0;
      ok = q >= v.n_ext && !(keep && keep[q]) && P.root[q] == q && strided_ok[q] && last_reader[q] == i && prod[q] >= 0;
      if (!ok) break;
      const Op &p = v.op(prod[q]);
      // writers that can store through a stride: conv epilogue (compiled shapes), BatchNorm apply, UnPooling gather;
      // in backward the producer reads the buffer's gradient through the same stride (dX conv, dW, BN, gather_sum)
      ok = (p.is_conv() && strided_conv_ok(p)) || p.type == OP_BN || p.type == OP_UNPOOL;
    }
    if (!ok || o.in0 == o.in1) continue;
    if (P.bf16() && (o.cin & 1)) continue;   // bf16 rows: the second input's columns must start dword-aligned (16-byte chunk loads)
    P.join_view[i] = 1;
    P.skip[i] = 1;
    P.root[o.in0] = o.out;
    P.col[o.in0] = 0;
    P.root[o.in1] = o.out;
    P.col[o.in1] = o.cin;        // cin = channels of in0
  }
  for (int b = 0; b < v.nbuf; ++b) {   // nested joins: resolve to the outermost storage
    int r = b, c = 0;
    while (P.root[r] != r) {
      c += P.col[r];
      r = P.root[r];
    }
    P.root[b] = r;
    P.col[b] = c;
    P.ld[b] = row_ld(r);
  }
  plan_bn_folds(v, readers, P);
}

// arena layout: [buffers (in-place JoinTable inputs own no storage)..., per-op areas (BatchNorm: mean/invstd;
// up-sampling conv: its 64 pre-summed weight slices)..., backward scratch: 2 x largest buffer, up-sampling weight
// gradient + its split data-gradient rows]
struct Layout {
  std::vector<int64_t> buf_off, buf_floats, aux_off;
  int64_t max_buf = 0, total = 0, fwd_total = 0, scratch0 = 0, scratch1 = 0, bextra = 0;
  // bf16 layout: an external read by anything but CONCAT_IN gets a bf16 copy in the arena (shadow), converted in front of
  // its first reader (first[b]); first[] holds the first op touching every storage root
  std::vector<char> shadow;
  std::vector<int> first;
};

// per-op area (floats).  fp32 layouts: BatchNorm's saved mean / invstd, the up-sampling convolution's 64 pre-summed
// weight slices.  bf16 layout: the convolutions' bf16 weight fragments, the up-sampling convolution's pre-summed fp32
// slices in front of its fragments; BatchNorm needs none (eval only: running statistics)
int64_t aux_floats(const Op &o, Kind kind) {
  const int64_t slices = round64(64 * (int64_t)o.cin * o.cout);
  if (kind == INFERENCE_BF16) {
    if (o.is_conv()) return round64(sgnn_bf16_wfrag_bytes(o.cin, o.cout, o.K(), 1) / 4);
    return o.type == OP_EXPAND ? slices + round64(sgnn_bf16_wfrag_bytes(o.cin, o.cout, 8, 8) / 4) : 0;
  }
  return o.type == OP_BN ? round64(2 * (int64_t)o.cin) : o.type == OP_EXPAND ? slices : 0;
}

// the per-op areas, from float `off` of the arena on; returns the float behind them
int64_t place_aux(const View &v, Kind kind, Layout &L, int64_t off) {
  for (int i = 0; i < v.nops; ++i) {
    const int64_t a = aux_floats(v.op(i), kind);
    if (a <= 0) continue;
    L.aux_off[i] = off;
    off += a;
  }
  return off;
}

// Inference layout (no backward pass will read the arena): a buffer's storage is handed to later buffers once its last
// reader has run.  Storage roots are allocated at the first op that writes into them (an in-place JoinTable's inputs
// write into the join buffer), released after the last op that touches them, outputs (`keep`) never; first-fit over an
// offset-ordered free list, so the arena is the high-water mark of the live set instead of the sum of all buffers —
// 3-4x smaller for a FullyConvolutionalNet stage (what bounds whole-scene inference, BASELINE configs[3]).
int make_layout_infer(const View &v, const Plan &P, const int32_t *keep, Layout &L) {
  const int never = v.nops + 1;
  std::vector<int> first(v.nbuf, never), last(v.nbuf, -1);
  auto in_arena = [&](int b) { return b >= v.n_ext || L.shadow[b]; };
  for (int i = 0; i < v.nops; ++i) {
    auto touch = [&](int b) {
      if (b < 0 || b >= v.nbuf || !in_arena(b)) return;
      const int r = P.root[b];
      if (i < first[r]) first[r] = i;
      if (i > last[r]) last[r] = i;
    };
    v.op(i).for_inputs(touch);
    touch(P.add_dst[i] >= 0 ? P.add_dst[i] : v.op(i).out);   // fused AddTable: the convolution writes the sum buffer itself
  }
  for (int b = v.n_ext; b < v.nbuf; ++b)
    if (keep && keep[b]) last[P.root[b]] = never;
  std::vector<std::pair<int64_t, int64_t>> free_list;   // (offset, floats), ordered by offset, neighbours merged
  int64_t top = place_aux(v, P.kind, L, 0);             // per-op areas first: small and alive for the whole call
  auto release = [&](int64_t o, int64_t n) {
    if (n <= 0) return;
    size_t k = 0;
    while (k < free_list.size() && free_list[k].first < o) ++k;
    free_list.insert(free_list.begin() + k, std::make_pair(o, n));
    if (k + 1 < free_list.size() && free_list[k].first + free_list[k].second == free_list[k + 1].first) {
      free_list[k].second += free_list[k + 1].second;
      free_list.erase(free_list.begin() + k + 1);
    }
    if (k > 0 && free_list[k - 1].first + free_list[k - 1].second == free_list[k].first) {
      free_list[k - 1].second += free_list[k].second;
      free_list.erase(free_list.begin() + k);
    }
  };
  auto take = [&](int64_t n) -> int64_t {
    if (n <= 0) return 0;
    size_t best = free_list.size();
    for (size_t k = 0; k < free_list.size(); ++k)
      if (free_list[k].second >= n && (best == free_list.size() || free_list[k].second < free_list[best].second)) best = k;
    if (best < free_list.size()) {
      const int64_t o = free_list[best].first;
      free_list[best].first += n;
      free_list[best].second -= n;
      if (free_list[best].second == 0) free_list.erase(free_list.begin() + best);
      return o;
    }
    if (!free_list.empty() && free_list.back().first + free_list.back().second == top) {   // grow the block at the top
      const int64_t o = free_list.back().first;
      free_list.pop_back();
      top = o + n;
      return o;
    }
    const int64_t o = top;
    top += n;
    return o;
  };
  for (int i = 0; i < v.nops; ++i) {
    for (int b = 0; b < v.nbuf; ++b)      // everything whose last toucher ran before this op
      if (in_arena(b) && P.root[b] == b && L.buf_off[b] >= 0 && last[b] == i - 1) release(L.buf_off[b], round64(L.buf_floats[b]));
    for (int b = 0; b < v.nbuf; ++b)
      if (in_arena(b) && P.root[b] == b && first[b] == i) L.buf_off[b] = take(round64(L.buf_floats[b]));
  }
  for (int b = v.n_ext; b < v.nbuf; ++b) {
    if (P.root[b] == b && L.buf_off[b] < 0) L.buf_off[b] = 0;   // never touched (a fused-away convolution output)
  }
  for (int b = v.n_ext; b < v.nbuf; ++b)   // (bf16: col counts elements — the executor adds it in bytes, see forward_bf16)
    if (P.root[b] != b) L.buf_off[b] = P.bf16() ? L.buf_off[P.root[b]] : L.buf_off[P.root[b]] + P.col[b];
  L.first = first;
  L.fwd_total = L.total = top;
  L.scratch0 = L.scratch1 = L.bextra = top;
  return 0;
}

// the layout of P.kind (keep: the buffers the caller reads; the inference layouts never recycle them)
int make_layout(const View &v, const Plan &P, Layout &L, const int32_t *keep) {
  L.buf_off.assign(v.nbuf, -1);
  L.buf_floats.resize(v.nbuf);
  L.aux_off.assign(v.nops, -1);
  L.shadow.assign(v.nbuf, 0);
  for (int b = 0; b < v.nbuf; ++b) {
    const int lev = v.bufs[2 * b], ch = v.bufs[2 * b + 1];
    if (lev < 0 || lev >= v.nlev || ch < 1) return -1;
    const int64_t elems = v.lev_n[lev] * (int64_t)(P.root[b] == b ? P.ld[b] : ch);   // (fp32: a root's ld is its channels)
    L.buf_floats[b] = P.f32[b] ? elems : (elems + 1) / 2;     // bf16: two elements per float of the arena
    if (L.buf_floats[b] > L.max_buf) L.max_buf = L.buf_floats[b];
  }
  if (P.kind != TRAINING) {
    if (P.bf16())
      for (int i = 0; i < v.nops; ++i) {
        if (v.op(i).type == OP_CONCAT_IN) continue;      // reads the fp32 externals itself
        v.op(i).for_inputs([&](int b) {
          if (b >= 0 && b < v.n_ext) L.shadow[b] = 1;
        });
      }
    return make_layout_infer(v, P, keep, L);
  }
  int64_t off = 0;
  for (int b = v.n_ext; b < v.nbuf; ++b) {
    if (P.root[b] != b) continue;
    L.buf_off[b] = off;
    off += round64(L.buf_floats[b]);
  }
  for (int b = v.n_ext; b < v.nbuf; ++b)
    if (P.root[b] != b) L.buf_off[b] = L.buf_off[P.root[b]] + P.col[b];
  off = place_aux(v, TRAINING, L, off);
  int64_t bextra = 0;
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    if (o.type != OP_EXPAND) continue;
    const int64_t need = aux_floats(o, TRAINING) + round64(v.lev_n[o.lev] * EXPAND_DX_SPLIT * (int64_t)o.cin);
    if (need > bextra) bextra = need;
  }
  L.fwd_total = off;       // what a forward pass touches: buffers + per-op areas
  L.scratch0 = off;
  off += round64(L.max_buf);
  L.scratch1 = off;
  off += round64(L.max_buf);
  L.bextra = off;
  off += bextra;
  L.total = off;
  return 0;
}

inline int64_t expand_dwc_bytes(int cin, int cout) { return (64 * (int64_t)cin * cout * 4 + 255) & ~int64_t(255); }

int64_t dw_slice(const View &v, int i) {   // workspace slice of op i's weight-gradient partials (256-byte multiple)
  const Op &o = v.op(i);
  int64_t w = 0;
  if (o.is_conv()) w = sgnn_conv_bwd_weight_ws_bytes(ConvSetup(v, o).n_out, o.K(), o.cin, o.cout);
  if (o.type == OP_EXPAND)   // partials + the 64 reduced slices themselves (they must not live in the shared gradient arena:
                             // with a deferred lane join the next program's backward pass would overwrite them)
    w = ((sgnn_conv_bwd_weight_ws_bytes(v.lev_n[o.lev], 64, o.cin, o.cout) + 255) & ~int64_t(255)) + expand_dwc_bytes(o.cin, o.cout);
  return (w + 255) & ~int64_t(255);
}

// every convolution keeps its weight-gradient partials in its own slice (their reduces run as one launch at the end)
int64_t dw_ws_need(const View &v) {
  int64_t need = 0;
  for (int i = 0; i < v.nops; ++i) need += dw_slice(v, i);
  return need;
}

int64_t ws_main(const View &v) {
  int64_t need = 0;
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    int64_t w = 0;
    if (o.type == OP_BN) w = sgnn_bn_ws_bytes(v.lev_n[o.lev], o.cin);
    if (o.type == OP_LINEAR) w = sgnn_linear_ws_bytes(v.lev_n[o.lev], o.cin, o.cout);
    if (w > need) need = w;
  }
  const int64_t dw = dw_ws_need(v);     // without a side lane the partial slices live in the main workspace too
  if (dw > need) need = dw;
  return (need + 255) & ~int64_t(255);
}

// statistics partials a convolution epilogue hands to the neighbouring BatchNorm: [grid blocks][2][C] doubles,
// placed behind the main workspace (the BatchNorm kernels use the main part while they read these)
int64_t ws_stats(const View &v) {
  int64_t need = 0;
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    if (!o.is_conv()) continue;
    const ConvSetup cs(v, o);
    // block counts of the finest-grained kernel that may run (the 16-row small kernel)
    const int64_t a = ((cs.n_out > 0 ? cs.n_out : 1) + 15) / 16 * 2 * o.cout * (int64_t)sizeof(double);   // forward: out rows x cout
    const int64_t b = ((cs.n > 0 ? cs.n : 1) + 15) / 16 * 2 * o.cin * (int64_t)sizeof(double);            // data gradient: in rows x cin
    if (a > need) need = a;
    if (b > need) need = b;
  }
  return (need + 255) & ~int64_t(255);
}

// a program that may fold a BatchNorm gets two tables: a convolution that sums the table of a folded BatchNorm in its prologue
// writes its own partials into the other one (sized from the ops alone: the sizing entry point knows neither readers nor layout)
bool may_fold(const View &v) {
  if (!g_fuse || !g_bn_fold || !g_tune.bn_fuse) return false;
  for (int i = 0; i + 1 < v.nops; ++i)
    if (fold_candidate(v, i)) return true;
  return false;
}
int64_t ws_need(const View &v) { return ws_main(v) + (may_fold(v) ? 2 : 1) * ws_stats(v); }

// weight-gradient lane: sgnn_prog_backward can run every dW (+ its reduce) on a second stream with its own
// workspace, concurrently with the dX / BatchNorm chain that forms the critical path (both only READ dy)
struct SideLane {
  hipStream_t stream = nullptr;
  void *ws = nullptr;
  int64_t ws_bytes = 0;
  hipEvent_t fork = nullptr, join = nullptr;
} g_side;
// The lane (its workspace and its two events) is one per process = one per GPU.  A backward call holds g_side_mu while
// it issues work; a second host thread that calls sgnn_prog_backward at the same time does not get the lane (its weight
// gradients run on its own stream and workspace — correct, just not overlapped), and sgnn_prog_set_side_stream waits
// for a call in flight before it swaps the lane.
std::mutex g_side_mu;
// sgnn_prog_defer_join(1): a backward call no longer makes its stream wait for the lane at its end — the CALLER joins the
// lane's stream before anything reads parameter gradients.  A program's last weight gradient (its first, widest
// convolution) otherwise stalls the dependent chain of the next program for as long as it runs.
bool g_defer_join = false;

#define PROG_TRY(call)           \
  do {                           \
    const int rc_ = (call);      \
    if (rc_ != SGNN_OK) return rc_; \
  } while (0)

// What one executor call works on: the caller's descriptors and pointer tables, and what plan and layout make of them.
// Where a buffer's storage is differs per pass (fp32 or bf16 arena, activations or gradients) and stays with the pass.
struct Ctx {
  View v;
  void *const *params, *const *idx, *const *lev_cnt;
  int nparams, nidx, training;
  void *ws;
  int64_t ws_bytes;
  sgnn_stream_t stream;
  Plan P;
  Layout L;
  // fp32 passes: the statistics partials a convolution epilogue has left for BatchNorm op i (pre[i], pre_nblk[i] blocks)
  std::vector<const double *> pre;
  std::vector<int64_t> pre_nblk;
  double *stats_ws, *stats_ws2;

  // plan and layout of these descriptors; false: they do not describe a program
  bool prepare(Kind kind, const int32_t *keep) {
    make_plan(v, keep, P, kind);
    if (make_layout(v, P, L, keep) != 0) return false;
    pre = std::vector<const double *>(v.nops, nullptr);
    pre_nblk = std::vector<int64_t>(v.nops, 0);
    stats_ws = (double *)((char *)ws + ws_main(v));
    stats_ws2 = (double *)((char *)stats_ws + ws_stats(v));
    return true;
  }
  int ch(int b) const { return b < 0 ? 0 : v.bufs[2 * b + 1]; }
  int cls(int b) const { return v.bufs[2 * b]; }
  int64_t rows(int b) const { return v.lev_n[cls(b)]; }
  int64_t ld(int b) const { return P.ld[b]; }       // row stride (elements): wider than the channels for a view
  float *param(int p) const { return (p >= 0 && p < nparams) ? (float *)params[p] : nullptr; }
  const int32_t *index(int i) const { return (i >= 0 && i < nidx && idx) ? (const int32_t *)idx[i] : nullptr; }
  // capacity mode: device row count of a rows class (NULL: lev_n is exact)
  const int64_t *count(int c) const { return (lev_cnt && c >= 0 && c < v.nlev) ? (const int64_t *)lev_cnt[c] : nullptr; }
  // the stride-2 tables and everything of the coarser levels (hash, 3x3x3 rulebooks, row counts) may still be in
  // flight on the caller's pyramid lane: the first Convolution(2,2) is the first operation that touches them
  // BatchNorm op i as the convolution it is folded into applies it; save: the layer's mean / invstd area
  ConvPre conv_pre(int i, float *save, bool forward) const {
    const Op &b = v.op(i);
    ConvPre p{};
    if (forward && training) {
      p.fuse.partial = pre[i];
      p.fuse.nblk = (int)pre_nblk[i];
    }
    p.fuse.eps = v.opf[4 * i];
    p.fuse.momentum = v.opf[4 * i + 1];
    p.fuse.running_mean = param(b.par + 2);
    p.fuse.running_var = param(b.par + 3);
    p.fuse.save_mean = save;
    p.fuse.save_invstd = save + b.cin;
    p.gamma = param(b.par);
    p.beta = param(b.par + 1);
    p.leak = v.opf[4 * i + 2];
    p.n_bn = v.lev_n[b.lev];
    p.n_bn_dev = count(b.lev);
    return p;
  }
  int wait_once(void *&wait_event) const {
    if (!wait_event) return SGNN_OK;
    sgnn_stamp("down-wait<", stream);
    SGNN_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)wait_event, 0));
    sgnn_stamp("down-wait>", stream);
    wait_event = nullptr;
    return SGNN_OK;
  }
};

}  // namespace

// stream2 == NULL switches the lane off.  ws2 must not be used by anything else while a backward call is in flight.
SGNN_EXPORT int sgnn_prog_set_side_stream(sgnn_stream_t stream2, void *ws2, int64_t ws2_bytes) {
  std::lock_guard<std::mutex> hold(g_side_mu);
  if (stream2 && !g_side.fork) {
    SGNN_HIP_TRY(hipEventCreateWithFlags(&g_side.fork, hipEventDisableTiming));
    SGNN_HIP_TRY(hipEventCreateWithFlags(&g_side.join, hipEventDisableTiming));
  }
  g_side.stream = (hipStream_t)stream2;
  g_side.ws = stream2 ? ws2 : nullptr;
  g_side.ws_bytes = stream2 ? ws2_bytes : 0;
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_prog_defer_join(int on) {
  const int prev = g_defer_join ? 1 : 0;
  g_defer_join = on != 0;
  return prev;
}

// mode 0: the gradient arena of sgnn_prog_backward (buffers + per-op areas + backward scratch); 1: the arena of
// sgnn_prog_forward (buffers + per-op areas); 2: the forward arena of an inference call (training = 2: liveness-packed);
// 3: the same with bf16 storage (training = 2 | 4)
SGNN_EXPORT int64_t sgnn_prog_arena_floats(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext,
                                           const int64_t *lev_n, int nlev, const int32_t *keep, int mode) {
  View v{ops, nullptr, nops, bufs, nbuf, n_ext, lev_n, nullptr, nullptr, nullptr, nullptr, nullptr, nlev};
  if (mode < 0 || mode > 3) return -1;
  Plan P;
  make_plan(v, keep, P, kind_of_mode(mode));
  Layout L;
  if (make_layout(v, P, L, keep) != 0) return -1;
  return mode == 0 ? L.total : L.fwd_total;
}

SGNN_EXPORT int64_t sgnn_prog_ws_bytes(const int32_t *ops, int nops, const int64_t *lev_n, int nlev) {
  View v{ops, nullptr, nops, nullptr, 0, 0, lev_n, nullptr, nullptr, nullptr, nullptr, nullptr, nlev};
  return ws_need(v);
}

// float offset of buffer `b` inside an arena (so the host layer can hand out views); -1 for externals, except that the
// bf16 layout reports where an external's bf16 copy lives (-1 if it has none).  infer: 0 training layout, 1 inference
// layout, 2 bf16 inference layout (rows of round-up-to-8 bf16 elements; LINEAR outputs stay fp32)
SGNN_EXPORT int64_t sgnn_prog_buffer_offset(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext,
                                            const int64_t *lev_n, int nlev, const int32_t *keep, int infer, int b) {
  View v{ops, nullptr, nops, bufs, nbuf, n_ext, lev_n, nullptr, nullptr, nullptr, nullptr, nullptr, nlev};
  if (infer < 0 || infer > 2) return -1;
  const Kind kind = infer == 2 ? INFERENCE_BF16 : infer == 1 ? INFERENCE : TRAINING;
  Plan P;
  make_plan(v, keep, P, kind);
  Layout L;
  if (make_layout(v, P, L, keep) != 0 || b < 0 || b >= nbuf) return -1;
  if (b < n_ext) return L.shadow[b] ? L.buf_off[b] : -1;
  return P.root[b] == b ? L.buf_off[b] : -1;      // buffers the caller keeps are never views
}

// What make_plan decides for these descriptors under the current switches, for tests and diagnostics: host only, nothing
// is launched.  mode as in sgnn_prog_arena_floats (3: the plan of the bf16 layout).  out: int32[4 * nops + 3 * nbuf] =
// per op {skip, add_dst, join_view, lin_bn}, then per buffer {root, col, ld}.
SGNN_EXPORT int sgnn_prog_plan(const int32_t *ops, int nops, const int32_t *bufs, int nbuf, int n_ext, const int64_t *lev_n,
                               int nlev, const int32_t *keep, int mode, int32_t *out) {
  SGNN_CHECK_ARG(ops && bufs && lev_n && out && nops >= 0 && nbuf >= 1 && nlev >= 1 && n_ext >= 0 && n_ext <= nbuf &&
                 mode >= 0 && mode <= 3);
  View v{ops, nullptr, nops, bufs, nbuf, n_ext, lev_n, nullptr, nullptr, nullptr, nullptr, nullptr, nlev};
  Plan P;
  make_plan(v, keep, P, kind_of_mode(mode));
  for (int i = 0; i < nops; ++i) {
    out[4 * i] = P.skip[i];
    out[4 * i + 1] = P.add_dst[i];
    out[4 * i + 2] = P.join_view[i];
    out[4 * i + 3] = P.lin_bn[i];
  }
  for (int b = 0; b < nbuf; ++b) {
    out[4 * nops + 3 * b] = P.root[b];
    out[4 * nops + 3 * b + 1] = P.col[b];
    out[4 * nops + 3 * b + 2] = (int32_t)P.ld[b];
  }
  return SGNN_OK;
}

// The forward pass of the bf16 inference layout (training = 2 | 4; infer_bf16.hip): the same plan — fused conv ->
// AddTable, in-place JoinTable views — over bf16 rows (row strides rounded up to 8 elements).  Externals stay the
// caller's fp32 tensors: CONCAT_IN converts while it gathers, any other reader gets a bf16 shadow copy made in front of
// its first reader.  LINEAR heads write fp32 logits.  Eval only (running statistics).
static int forward_bf16(const Ctx &c, void *const *ext, float *arena, void *wait_event) {
  const View &v = c.v;
  const Plan &PL = c.P;
  const Layout &L = c.L;
  const sgnn_stream_t stream = c.stream;
  const int n_ext = v.n_ext, nbuf = v.nbuf, nlev = v.nlev;
  // storage of buffer b: the caller's tensor, or its root's arena slot + its column offset (bf16 elements)
  auto B = [&](int b) -> void * {
    if (b < 0) return nullptr;
    if (b < n_ext && !L.shadow[b]) return ext[b];
    const int r = PL.root[b];
    return (char *)arena + 4 * L.buf_off[r] + (PL.f32[r] ? 4 : 2) * (int64_t)PL.col[b];
  };
  auto EXT = [&](int b) -> const float * { return b < 0 ? nullptr : (const float *)ext[b]; };
  for (int i = 0; i < v.nops; ++i) {
    const Op &o = v.op(i);
    const int in0 = o.in0, in1 = o.in1, out = o.out, par = o.par, lev = o.lev, cin = o.cin, cout = o.cout;
    SGNN_CHECK_ARG(out >= n_ext && out < nbuf && lev >= 0 && lev < nlev && in0 < nbuf && in1 < nbuf);
    SGNN_CHECK_ARG(o.type == OP_CONCAT_IN || in0 >= 0);
    SGNN_CHECK_ARG(o.type == OP_LINEAR || !PL.f32[out]);
    const int64_t n = v.lev_n[lev];
    for (int b = 0; b < n_ext; ++b)       // bf16 copies of the externals this op is the first to read
      if (L.shadow[b] && L.first[b] == i)
        PROG_TRY(sgnn_bf16_concat3(EXT(b), c.ch(b), nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, c.rows(b), B(b), c.ld(b),
                                   c.count(c.cls(b)), stream));
    if (PL.skip[i]) continue;
    if (o.type == OP_CONV_DOWN) PROG_TRY(c.wait_once(wait_event));
    switch (o.type) {
      case OP_CONV_SUBM:
      case OP_CONV_DOWN: {
        const ConvSetup cs(v, o);
        SGNN_CHECK_ARG(cs.ok);
        int dst = out;
        const void *addend = nullptr;
        int64_t ld_add = 0;
        if (PL.add_dst[i] >= 0) {           // fused AddTable: the sum is stored, the convolution's own output never is
          addend = B(PL.add_src[i]);
          ld_add = c.ld(PL.add_src[i]);
          dst = PL.add_dst[i];
        }
        void *wf = arena + L.aux_off[i];
        PROG_TRY(sgnn_bf16_conv_prepare(c.param(par), cin, cout, cs.K, 1, wf, stream));
        PROG_TRY(sgnn_bf16_conv_run(B(in0), c.rows(in0), cin, c.ld(in0), c.param(par), wf, cs.K, cs.tab_f, cs.ld_f, cs.n_out, cout,
                                    B(dst), c.ld(dst), addend, ld_add, nullptr, 1, cs.K, c.count(cs.cnt_class), stream));
        break;
      }
      case OP_UNPOOL:
        SGNN_CHECK_ARG(lev + 1 < nlev);
        PROG_TRY(sgnn_bf16_gather_rows(B(in0), c.ld(in0), cin, (const int32_t *)v.lev_parent[lev], n, B(out), c.ld(out),
                                       c.count(lev), stream));
        break;
      case OP_BN:
        PROG_TRY(sgnn_bf16_bn_eval(B(in0), c.ld(in0), n, cin, c.param(par), c.param(par + 1), c.param(par + 2), c.param(par + 3),
                                   v.opf[4 * i], v.opf[4 * i + 2], B(out), c.ld(out), c.count(lev), stream));
        break;
      case OP_ADD:
        SGNN_CHECK_ARG(in1 >= 0);
        PROG_TRY(sgnn_bf16_add(B(in0), c.ld(in0), B(in1), c.ld(in1), n, cin, B(out), c.ld(out), c.count(lev), stream));
        break;
      case OP_JOIN:
        SGNN_CHECK_ARG(in1 >= 0);
        PROG_TRY(sgnn_bf16_join(B(in0), c.ld(in0), cin, B(in1), c.ld(in1), cout, n, B(out), c.ld(out), c.count(lev), stream));
        break;
      case OP_CONCAT_IN: {
        const int in2 = o.in2;
        SGNN_CHECK_ARG(in2 < nbuf && in0 < n_ext && in1 < n_ext && in2 < n_ext && c.ch(in0) + c.ch(in1) + c.ch(in2) == c.ch(out));
        PROG_TRY(sgnn_bf16_concat3(EXT(in0), c.ch(in0), c.index(o.ia), EXT(in1), c.ch(in1), c.index(o.ib), EXT(in2), c.ch(in2),
                                   c.index(o.ic), n, B(out), c.ld(out), c.count(lev), stream));
        break;
      }
      case OP_EXPAND:
        SGNN_CHECK_ARG(c.rows(out) == 8 * n);
        PROG_TRY(sgnn_bf16_conv_expand_impl(B(in0), n, cin, c.ld(in0), c.param(par), (const int32_t *)v.lev_nbr[lev], v.lev_ld[lev],
                                            cout, B(out), c.ld(out), c.count(lev), arena + L.aux_off[i], stream));
        break;
      case OP_LINEAR: {
        SGNN_CHECK_ARG(cout >= 1 && cout <= 4 && PL.f32[out] && c.ld(out) == cout);
        const float *w[4] = {}, *b[4] = {};
        for (int q = 0; q < cout; ++q) {
          w[q] = c.param(par + 2 * q);
          b[q] = c.param(par + 2 * q + 1);
        }
        PROG_TRY(sgnn_bf16_linear_rows(B(in0), c.ld(in0), n, cin, w, b, cout, (float *)B(out), c.count(lev), stream));
        break;
      }
      default:
        sgnn_set_error("sgnn_prog_forward: unknown op %d", o.type);
        return SGNN_EINVAL;
    }
  }
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_prog_forward(const int32_t *ops, const float *opf, int nops, const int32_t *bufs, int nbuf, int n_ext,
                                  const int64_t *lev_n, const int64_t *lev_ld, void *const *lev_nbr,
                                  void *const *lev_children, void *const *lev_ptable, void *const *lev_parent,
                                  void *const *lev_cnt, int nlev, void *const *params, int nparams,
                                  void *const *ext, void *const *idx,
                                  int nidx, float *arena, int64_t arena_floats, const int32_t *keep, int training,
                                  void *wait_event, void *ws, int64_t ws_bytes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ops && opf && bufs && lev_n && lev_ld && params && arena && nops >= 0 && nbuf >= 1 && nlev >= 1 &&
                 n_ext >= 0 && n_ext <= nbuf && (n_ext == 0 || ext));
  // training: bit 0 batch statistics, bit 1 the inference layout (no backward call may follow), bit 2 bf16 storage
  const Kind kind = (training & 4) ? INFERENCE_BF16 : (training & 2) ? INFERENCE : TRAINING;
  if ((training & 4) && (training & 3) != 2) {
    sgnn_set_error("sgnn_prog_forward: bf16 storage needs the inference layout in eval mode (training = 2 | 4)");
    return SGNN_EINVAL;
  }
  training &= 1;
  Ctx c{View{ops, opf, nops, bufs, nbuf, n_ext, lev_n, lev_ld, lev_nbr, lev_children, lev_ptable, lev_parent, nlev},
        params, idx, lev_cnt, nparams, nidx, training, ws, ws_bytes, stream};
  SGNN_CHECK_ARG(c.prepare(kind, keep));
  const View &v = c.v;
  const Plan &PL = c.P;
  const Layout &L = c.L;
  if (arena_floats < L.fwd_total) {
    sgnn_set_error("sgnn_prog_forward: arena too small (%lld < %lld floats)", (long long)arena_floats,
                   (long long)L.fwd_total);
    return SGNN_ENOWS;
  }
  if (ws_bytes < ws_need(v)) {
    sgnn_set_error("sgnn_prog_forward: workspace too small");
    return SGNN_ENOWS;
  }
  if (kind == INFERENCE_BF16) return forward_bf16(c, ext, arena, wait_event);
  auto B = [&](int b) -> float * { return b < 0 ? nullptr : (b < n_ext ? (float *)ext[b] : arena + L.buf_off[b]); };
  // Epilogue fusions (same arithmetic, fewer passes and launches; planned by make_plan):
  //  * conv -> AddTable: the convolution adds the other AddTable input while it stores (the sum buffer is written
  //    directly, the convolution's own output buffer stays untouched) when nothing else reads the convolution output;
  //  * conv [-> AddTable] -> BatchNorm (training): the convolution epilogue reduces the column sums the BatchNorm
  //    statistics pass would recompute from HBM;
  //  * JoinTable in place: its inputs are written straight into their column range of the join buffer.
  for (int i = 0; i < nops; ++i) {
    const Op &o = v.op(i);
    const int in0 = o.in0, in1 = o.in1, out = o.out, par = o.par, lev = o.lev, cin = o.cin, cout = o.cout;
    SGNN_CHECK_ARG(out >= n_ext && out < nbuf && lev >= 0 && lev < nlev && in0 < nbuf && in1 < nbuf);
    SGNN_CHECK_ARG(o.type == OP_CONCAT_IN || in0 >= 0);
    const int64_t n = lev_n[lev];
    if (PL.skip[i]) continue;
    if (o.type == OP_CONV_DOWN) PROG_TRY(c.wait_once(wait_event));
    switch (o.type) {
      case OP_CONV_SUBM:
      case OP_CONV_DOWN: {
        const ConvSetup cs(v, o);
        SGNN_CHECK_ARG(cs.ok);
        ConvEpi epi{};
        int dst_buf = out;
        if (PL.add_dst[i] >= 0) {
          epi.addend = B(PL.add_src[i]);
          epi.ld_add = c.ld(PL.add_src[i]);
          dst_buf = PL.add_dst[i];
        }
        const int j = i + 1 + (PL.add_dst[i] >= 0 ? 1 : 0);
        if (g_fuse && training && cs.n_out > 0 && j < nops && v.op(j).type == OP_BN && v.op(j).in0 == dst_buf &&
            sgnn_conv_epi_supported(cin, cout)) {
          epi.stats = 1;
          // (a folded BatchNorm's table is read by every workgroup of this launch while the others store their partials)
          epi.partial = (PL.pre_bn[i] >= 0 && c.pre[PL.pre_bn[i]] == c.stats_ws) ? c.stats_ws2 : c.stats_ws;
          c.pre[j] = epi.partial;
          c.pre_nblk[j] = sgnn_conv_grid_blocks(cs.n_out, cin, cout, cs.K);
        }
        epi.ldy = c.ld(dst_buf);
        epi.n_dev = c.count(cs.cnt_class);
        if (PL.pre_bn[i] >= 0) {             // the BatchNormReLU in front of it was not run: its INPUT rows are gathered
          const int bi = PL.pre_bn[i];
          const ConvPre cp = c.conv_pre(bi, arena + L.aux_off[bi], true);
          if (training && !cp.fuse.partial) {
            sgnn_set_error("sgnn_prog_forward: a folded BatchNorm has no statistics partials");
            return SGNN_EINVAL;
          }
          const int bin = v.op(bi).in0;
          epi.ldx = c.ld(bin);
          PROG_TRY(sgnn_conv_fwd_impl(B(bin), n, cin, c.param(par), cs.K, cs.tab_f, cs.ld_f, cs.n_out, cout, B(dst_buf), 0, 0,
                                      nullptr, nullptr, 1, 1, cs.K, &epi, stream, &cp));
          break;
        }
        epi.ldx = c.ld(in0);
        PROG_TRY(sgnn_conv_fwd_impl(B(in0), n, cin, c.param(par), cs.K, cs.tab_f, cs.ld_f, cs.n_out, cout, B(dst_buf), 0, 0,
                                    nullptr, nullptr, 1, 1, cs.K, &epi, stream));
        break;
      }
      case OP_UNPOOL:  // in0 lives on level lev+1, out on level lev
        SGNN_CHECK_ARG(lev + 1 < nlev);
        PROG_TRY(sgnn_gather_rows_ld(B(in0), c.ld(in0), cin, (const int32_t *)lev_parent[lev], n, B(out), c.ld(out), stream,
                                     c.count(lev)));
        break;
      case OP_BN: {
        if (PL.fold[i] >= 0) break;          // convolution fold[i] applies the layer (and stores its statistics)
        float *save = arena + L.aux_off[i];
        PROG_TRY(sgnn_bn_fwd_impl(B(in0), c.ld(in0), n, cin, c.param(par), c.param(par + 1), c.param(par + 2), c.param(par + 3),
                                  opf[4 * i], opf[4 * i + 1], training, opf[4 * i + 2], save, save + cin, B(out), c.ld(out),
                                  c.pre[i], c.pre_nblk[i], ws, ws_bytes, stream, c.count(lev)));
        break;
      }
      case OP_ADD:
        SGNN_CHECK_ARG(in1 >= 0);
        PROG_TRY(sgnn_add_ld(B(in0), c.ld(in0), B(in1), c.ld(in1), n, cin, B(out), c.ld(out), stream, c.count(lev)));
        break;
      case OP_JOIN:  // cin = channels of in0, cout = channels of in1
        SGNN_CHECK_ARG(in1 >= 0 && c.ld(in0) == cin && c.ld(in1) == cout && c.ld(out) == cin + cout);
        PROG_TRY(sgnn_concat_rows_dn(B(in0), cin, nullptr, B(in1), cout, nullptr, n, B(out), stream, c.count(lev)));
        break;
      case OP_CONCAT_IN: {
        const int in2 = o.in2;
        SGNN_CHECK_ARG(in2 < nbuf && c.ch(in0) + c.ch(in1) + c.ch(in2) == c.ch(out) && c.ld(out) == c.ch(out));
        PROG_TRY(sgnn_concat3_rows_dn(B(in0), c.ch(in0), c.index(o.ia), B(in1), c.ch(in1), c.index(o.ib), B(in2), c.ch(in2),
                                      c.index(o.ic), n, B(out), stream, c.count(lev)));
        break;
      }
      case OP_EXPAND: {   // out rows = 8 * n (child row 8p + parity), features of the parents never replicated
        SGNN_CHECK_ARG(c.rows(out) == 8 * n && c.ld(in0) == cin && c.ld(out) == cout);
        const int32_t *S, *ST, *PAR;
        PROG_TRY(sgnn_expand_maps(&S, &ST, &PAR));
        float *wc = arena + L.aux_off[i];
        PROG_TRY(sgnn_expand_weights(c.param(par), cin, cout, wc, stream));
        ConvEpi xepi{};
        xepi.n_dev = c.count(lev);
        PROG_TRY(sgnn_conv_fwd_impl(B(in0), n, cin, wc, 8, (const int32_t *)lev_nbr[lev], lev_ld[lev], n, cout, B(out), 0,
                                    0, S, nullptr, 1, 8, 27, &xepi, stream));
        break;
      }
      case OP_LINEAR: {
        SGNN_CHECK_ARG(cout >= 1 && cout <= 4 && c.ld(in0) == cin);
        const float *w[4] = {}, *b[4] = {};
        for (int q = 0; q < cout; ++q) {
          w[q] = c.param(par + 2 * q);
          b[q] = c.param(par + 2 * q + 1);
        }
        PROG_TRY(sgnn_linear_fwd_rows(B(in0), n, cin, w, b, cout, B(out), stream, c.count(lev)));
        break;
      }
      default:
        sgnn_set_error("sgnn_prog_forward: unknown op %d", o.type);
        return SGNN_EINVAL;
    }
  }
  return SGNN_OK;
}

namespace {

// Where the gradient of every buffer is while a backward call runs
struct Grads {
  // gradient state of a buffer: NONE nothing yet, HELD G(b) holds it, ALIAS it EQUALS the gradient of buffer alias[b]
  // (an AddTable input whose only contribution so far is the sum's gradient: nothing is copied until something
  // has to be added to it, and a reader just follows the alias), CALLER it is the caller's tensor gout[b], read in place
  // (contiguous rows; folded into G(b) by the first kernel that has to add to it — no up-front copy of the outputs'
  // gradients into the arena)
  enum State : char { NONE, HELD, ALIAS, CALLER };
  const Ctx &c;
  void *const *pgrads, *const *ext, *const *gext, *const *gout;
  const float *arena;
  float *garena;     // same layout as arena
  std::vector<State> state;
  std::vector<int> alias;
  std::vector<int> lazy_lin;   // buffer -> LINEAR op whose data gradient the buffer's BatchNorm forms itself (BnLin)
  std::vector<char> viewed;    // storage shared through an in-place JoinTable: keeps the copying path
  float *scratch[2];

  Grads(const Ctx &c_, void *const *pgrads_, void *const *ext_, void *const *gext_, void *const *gout_, const float *arena_,
        float *garena_)
      : c(c_), pgrads(pgrads_), ext(ext_), gext(gext_), gout(gout_), arena(arena_), garena(garena_),
        state(c_.v.nbuf, NONE), alias(c_.v.nbuf, -1), lazy_lin(c_.v.nbuf, -1), viewed(c_.v.nbuf, 0),
        scratch{garena_ + c_.L.scratch0, garena_ + c_.L.scratch1} {
    for (int b = 0; b < c.v.nbuf; ++b)
      if (c.P.root[b] != b) viewed[b] = viewed[c.P.root[b]] = 1;
  }
  // activations and gradient slot of buffer b (row stride of both: c.ld(b)); gradient of parameter p
  const float *X(int b) const { return b < 0 ? nullptr : (b < c.v.n_ext ? (const float *)ext[b] : arena + c.L.buf_off[b]); }
  float *G(int b) const { return b < c.v.n_ext ? (float *)gext[b] : garena + c.L.buf_off[b]; }
  float *PG(int p) const { return (p >= 0 && p < c.nparams) ? (float *)pgrads[p] : nullptr; }
  bool wants(int b) const { return b >= c.v.n_ext || gext[b] != nullptr; }
  bool has(int b) const { return state[b] != NONE; }
  // where the gradient a buffer HOLDS lives (its own arena slot, or the caller's tensor) and that storage's row stride
  const float *held(int b) const { return state[b] == CALLER ? (const float *)gout[b] : G(b); }
  int64_t held_ld(int b) const { return state[b] == CALLER ? (int64_t)c.ch(b) : c.ld(b); }
  // where b's gradient is read
  const float *read(int b) const { return state[b] == ALIAS ? held(alias[b]) : held(b); }
  int64_t read_ld(int b) const { return state[b] == ALIAS ? held_ld(alias[b]) : held_ld(b); }
  // a kernel has written the complete gradient of b into G(b)
  void written(int b) {
    state[b] = HELD;
    alias[b] = -1;
  }
  // where a kernel should write the gradient of buffer b: the buffer itself unless it already holds data
  float *target(int b, int which) const { return state[b] == HELD ? scratch[which] : G(b); }
  int64_t target_ld(int b, const float *t) const { return t == G(b) ? c.ld(b) : c.ch(b); }   // scratch rows are contiguous
  int commit(int b, float *wrote) {  // fold a freshly written gradient into buffer b
    const int64_t n = c.rows(b);
    const int ch = c.ch(b);
    const int64_t *cnt = c.count(c.cls(b));
    if (wrote != G(b)) return sgnn_add_ld(G(b), c.ld(b), wrote, ch, n, ch, G(b), c.ld(b), c.stream, cnt);
    if (state[b] == ALIAS || state[b] == CALLER) {            // G(b) = fresh + the aliased / the caller's gradient
      const float *other = read(b);
      const int64_t ldo = read_ld(b);
      written(b);
      return sgnn_add_ld(G(b), c.ld(b), other, ldo, n, ch, G(b), c.ld(b), c.stream, cnt);
    }
    written(b);
    return SGNN_OK;
  }
  // the caller's gradients of the program outputs: read in place where nothing has to be added into shared storage
  int adopt_outputs() {
    for (int b = c.v.n_ext; b < c.v.nbuf; ++b) {
      if (!gout[b]) continue;
      if (viewed[b] || !g_fuse) {
        if (c.L.buf_floats[b] > 0) PROG_TRY(sgnn_copy_words(G(b), gout[b], c.L.buf_floats[b], (hipStream_t)c.stream));
        state[b] = HELD;
      } else {
        state[b] = CALLER;
      }
    }
    return SGNN_OK;
  }
  int finish_externals() {
    for (int b = 0; b < c.v.n_ext; ++b) {                   // the caller reads gext[b]: an alias has to become a copy,
      if (!gext[b] || c.L.buf_floats[b] == 0) continue;     // an input nothing reached gets zeros
      if (state[b] == ALIAS)
        PROG_TRY(sgnn_copy_words(G(b), read(b), c.L.buf_floats[b], (hipStream_t)c.stream));
      else if (state[b] == NONE)
        PROG_TRY(sgnn_fill32(G(b), 0u, c.L.buf_floats[b], (hipStream_t)c.stream));
    }
    return SGNN_OK;
  }
};

// The weight-gradient side of one backward call: dW launches go to the side lane when one is configured and its workspace
// is big enough, otherwise to the call's own stream and workspace
struct Lane {
  struct PendingExpand { const float *dwc; int cin, cout; float *dw; };
  std::unique_lock<std::mutex> lock;
  hipStream_t hs;
  bool side, forked = false;
  char *ws;            // every op takes its dw_slice from here, at `off`
  int64_t off = 0;
  DwBatch batch{};
  std::vector<PendingExpand> pending_expand;

  Lane(const Ctx &c, hipStream_t hs_) : lock(g_side_mu, std::try_to_lock), hs(hs_) {
    side = lock.owns_lock() && g_side.stream && g_side.stream != hs && g_side.ws && g_side.ws_bytes >= dw_ws_need(c.v);
    ws = (char *)(side ? g_side.ws : c.ws);
    sgnn_dw_batch = side ? &batch : nullptr;   // without the lane the slices share `ws` with the BatchNorm kernels: reduce at once
  }
  ~Lane() { sgnn_dw_batch = nullptr; }         // the deferral is on only while this call runs, whatever path it leaves by
  hipStream_t stream() const { return side ? g_side.stream : hs; }
  hipStream_t fork() {
    if (!side) return hs;
    (void)hipEventRecord(g_side.fork, hs);                 // dy of this op is final here (all its consumers ran)
    (void)hipStreamWaitEvent(g_side.stream, g_side.fork, 0);
    forked = true;
    return g_side.stream;
  }
  int finish() {
    PROG_TRY(sgnn_dw_batch_flush(&batch, stream()));      // all deferred weight-gradient reduces: one launch
    for (const PendingExpand &pe : pending_expand)
      PROG_TRY(sgnn_expand_weights_bwd(pe.dwc, pe.cin, pe.cout, pe.dw, (sgnn_stream_t)stream()));
    if (forked && !g_defer_join) {                      // parameter gradients are complete once the lane has drained
      SGNN_HIP_TRY(hipEventRecord(g_side.join, g_side.stream));
      SGNN_HIP_TRY(hipStreamWaitEvent(hs, g_side.join, 0));
    }
    return SGNN_OK;
  }
};

// no gradient reached the output of op o: its parameters get zero gradients, its inputs nothing
int bwd_unreached(const Ctx &c, const Grads &g, const Op &o) {
  const hipStream_t hs = (hipStream_t)c.stream;
  if (o.is_conv() || o.type == OP_EXPAND) PROG_TRY(sgnn_fill32(g.PG(o.par), 0u, (int64_t)o.K() * o.cin * o.cout, hs));
  if (o.type == OP_BN) {
    void *zp[2] = {g.PG(o.par), g.PG(o.par + 1)};
    const int64_t zw[2] = {o.cin, o.cin};
    PROG_TRY(sgnn_fill32_multi(zp, zw, 2, 0u, hs));
  }
  if (o.type == OP_LINEAR)
    for (int q = 0; q < o.cout; ++q) {
      void *zp[2] = {g.PG(o.par + 2 * q), g.PG(o.par + 2 * q + 1)};
      const int64_t zw[2] = {o.cin, 1};
      PROG_TRY(sgnn_fill32_multi(zp, zw, 2, 0u, hs));
    }
  return SGNN_OK;
}

int bwd_conv(Ctx &c, Grads &g, Lane &lane, int i) {
  const Op &o = c.v.op(i);
  const ConvSetup cs(c.v, o);
  SGNN_CHECK_ARG(cs.ok);
  const int in0 = o.in0, cin = o.cin, cout = o.cout;
  const float *dy = g.read(o.out);
  const int64_t ld_dy = g.read_ld(o.out);
  // The lane forks HERE, in front of the data-gradient launch: the weight gradient runs beside the dX kernel of its layer.
  // (Never make the lane wait for a LATER kernel of the training stream: one such edge per program — no kernel moved —
  //  costs a replayed step +0.75 ms, profiles/r06l_ab_endfork.txt; every variant of round 3-6 that re-timed the forks lost
  //  0.8-0.9 ms the same way.)
  const hipStream_t ls = lane.fork();
  if (g.wants(in0)) {
    if (g_fuse && sgnn_conv_epi_supported(cout, cin) && cs.n > 0) {
      // the data gradient lands in G(in0) directly: what the buffer (or its alias) already holds is added in the
      // store (in place), and when in0 is the output of the BatchNormReLU right before this op and this is the
      // last contribution to its gradient, the epilogue also reduces sum dz / sum dz*xhat for that BatchNorm
      ConvEpi epi{};
      if (g.has(in0)) {                    // what the buffer (or its alias / the caller's tensor) already holds
        epi.addend = g.read(in0);
        epi.ld_add = g.read_ld(in0);
      }
      if (i > 0 && c.v.op(i - 1).type == OP_BN && c.v.op(i - 1).out == in0 && c.v.op(i - 1).cin == cin) {
        const Op &bo = c.v.op(i - 1);
        const float *save = g.arena + c.L.aux_off[i - 1];
        epi.stats = 2;
        epi.partial = c.stats_ws;
        epi.bn_x = g.X(bo.in0);
        epi.ld_bnx = c.ld(bo.in0);
        epi.mean = save;
        epi.invstd = save + cin;
        epi.gamma = c.param(bo.par);
        epi.beta = c.param(bo.par + 1);
        epi.leak = c.v.opf[4 * (i - 1) + 2];
        c.pre[i - 1] = c.stats_ws;
        c.pre_nblk[i - 1] = sgnn_conv_grid_blocks(cs.n, cout, cin, cs.K);
      }
      epi.ldx = ld_dy;
      epi.ldy = c.ld(in0);
      epi.n_dev = c.count(o.lev);
      PROG_TRY(sgnn_conv_fwd_impl(dy, cs.n_out, cout, c.param(o.par), cs.K, cs.tab_b, cs.ld_b, cs.n, cin, g.G(in0), cs.flags_b, 0,
                                  nullptr, nullptr, 1, 1, cs.K, &epi, c.stream));
      g.written(in0);
    } else {
      SGNN_CHECK_ARG(ld_dy == cout);               // views are only planned around compiled shapes
      float *t = g.target(in0, 0);
      ConvEpi pepi{};
      pepi.n_dev = c.count(o.lev);
      PROG_TRY(sgnn_conv_fwd_impl(dy, cs.n_out, cout, c.param(o.par), cs.K, cs.tab_b, cs.ld_b, cs.n, cin, t, cs.flags_b, 0, nullptr,
                                  nullptr, 1, 1, cs.K, &pepi, c.stream));
      PROG_TRY(g.commit(in0, t));
    }
  }
  const int64_t slice = dw_slice(c.v, i);
  if (c.P.pre_bn[i] >= 0) {   // in0 was never stored: the weight gradient applies the folded BatchNormReLU to that layer's input
    const int bi = c.P.pre_bn[i], bin = c.v.op(bi).in0;
    const ConvPre cp = c.conv_pre(bi, const_cast<float *>(g.arena) + c.L.aux_off[bi], false);
    PROG_TRY(sgnn_conv_bwd_weight_impl(g.X(bin), cs.n, cin, c.ld(bin), dy, cout, ld_dy, cs.tab_f, cs.ld_f, cs.K, cs.n_out,
                                       g.PG(o.par), 0, nullptr, nullptr, 1, 1, cs.K, lane.ws + lane.off, slice, (sgnn_stream_t)ls,
                                       c.count(cs.cnt_class), &cp));
  } else {
    PROG_TRY(sgnn_conv_bwd_weight_impl(g.X(in0), cs.n, cin, c.ld(in0), dy, cout, ld_dy, cs.tab_f, cs.ld_f, cs.K, cs.n_out,
                                       g.PG(o.par), 0, nullptr, nullptr, 1, 1, cs.K, lane.ws + lane.off, slice, (sgnn_stream_t)ls,
                                       c.count(cs.cnt_class)));
  }
  if (ls != lane.hs) sgnn_stamp("dw>", (sgnn_stream_t)ls);      // (nothing unless stamps are on: scripts/lane_stamps.py)
  lane.off += slice;
  return SGNN_OK;
}

int bwd_unpool(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  if (!g.wants(o.in0)) return SGNN_OK;
  float *t = g.target(o.in0, 0);
  PROG_TRY(sgnn_gather_sum_ld(g.read(o.out), g.read_ld(o.out), o.cin, (const int32_t *)c.v.lev_children[o.lev],
                              c.v.lev_ld[o.lev + 1], 8, c.v.lev_n[o.lev + 1], t, g.target_ld(o.in0, t), c.stream,
                              c.count(o.lev + 1)));
  return g.commit(o.in0, t);
}

int bwd_bn(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  const int in0 = o.in0, cin = o.cin;
  const float *save = g.arena + c.L.aux_off[i];
  // the kernel adds what the buffer already holds (in place) or the aliased gradient: no scratch pass, no k_add
  const float *addend = nullptr;
  int64_t ld_add = cin;
  if (g.wants(in0) && g.has(in0)) {
    addend = g.read(in0);
    ld_add = g.read_ld(in0);
  }
  float *t = g.wants(in0) ? g.G(in0) : g.scratch[0];
  BnLin bl{};
  const bool lazy = g.lazy_lin[o.out] >= 0;
  if (lazy) {                       // dy = (gradient of the head's output) x (the head's weights), never stored
    const Op &lo = c.v.op(g.lazy_lin[o.out]);
    bl.g = g.read(lo.out);
    bl.ldg = g.read_ld(lo.out);
    bl.nout = lo.cout;
    for (int q = 0; q < lo.cout; ++q) bl.w[q] = c.param(lo.par + 2 * q);
  }
  PROG_TRY(sgnn_bn_bwd_impl(g.X(in0), c.ld(in0), lazy ? nullptr : g.read(o.out), g.read_ld(o.out), c.v.lev_n[o.lev], cin,
                            c.param(o.par), c.param(o.par + 1), save, save + cin, c.training, c.v.opf[4 * i + 2], addend, ld_add,
                            t, g.wants(in0) ? c.ld(in0) : cin, g.PG(o.par), g.PG(o.par + 1), c.pre[i], c.pre_nblk[i], c.ws,
                            c.ws_bytes, c.stream, c.count(o.lev), lazy ? &bl : nullptr));
  if (g.wants(in0)) g.written(in0);
  return SGNN_OK;
}

int bwd_add(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  const int64_t n = c.v.lev_n[o.lev];
  const float *dy = g.read(o.out);
  const int64_t ld_dy = g.read_ld(o.out);
  const int src = g.state[o.out] == Grads::ALIAS ? g.alias[o.out] : o.out;      // the buffer that physically holds dy
  for (int b : {o.in0, o.in1}) {
    if (!g.wants(b)) continue;
    if (g.state[b] == Grads::HELD) {
      PROG_TRY(sgnn_add_ld(g.G(b), c.ld(b), dy, ld_dy, n, o.cin, g.G(b), c.ld(b), c.stream, c.count(o.lev)));
    } else if (g.has(b)) {            // two contributions held elsewhere: materialise the sum
      PROG_TRY(sgnn_add_ld(g.read(b), g.read_ld(b), dy, ld_dy, n, o.cin, g.G(b), c.ld(b), c.stream, c.count(o.lev)));
      g.written(b);
    } else {
      g.state[b] = Grads::ALIAS;
      g.alias[b] = src;
    }
  }
  return SGNN_OK;
}

int bwd_join(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  const int in0 = o.in0, in1 = o.in1;
  if (c.P.join_view[i]) {                                   // in place: the inputs' gradients ARE column ranges of dy
    if (g.state[o.out] != Grads::HELD || g.has(in0) || g.has(in1)) {
      sgnn_set_error("sgnn_prog_backward: in-place JoinTable met an unexpected gradient state");
      return SGNN_EINVAL;
    }
    g.written(in0);
    g.written(in1);
    return SGNN_OK;
  }
  const int64_t n = c.v.lev_n[o.lev];
  SGNN_CHECK_ARG(g.read_ld(o.out) == o.cin + o.cout && c.ld(in0) == o.cin && c.ld(in1) == o.cout);   // make_plan: a copying JoinTable never reads views
  float *ta = g.wants(in0) ? g.target(in0, 0) : nullptr;
  float *tb = g.wants(in1) ? g.target(in1, 1) : nullptr;
  PROG_TRY(sgnn_concat_rows_bwd_dn(g.read(o.out), o.cin, nullptr, o.cout, nullptr, n, ta, n, tb, n, c.stream, c.count(o.lev)));
  if (ta) PROG_TRY(g.commit(in0, ta));
  if (tb) PROG_TRY(g.commit(in1, tb));
  return SGNN_OK;
}

int bwd_concat_in(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  const int src[3] = {o.in0, o.in1, o.in2};
  float *d[3] = {nullptr, nullptr, nullptr};
  for (int q = 0; q < 3; ++q)
    if (src[q] >= 0 && g.wants(src[q])) {
      if (g.has(src[q])) {
        sgnn_set_error("sgnn_prog_backward: a CONCAT_IN source already carries a gradient (unsupported)");
        return SGNN_EINVAL;
      }
      d[q] = g.G(src[q]);
      g.written(src[q]);
    }
  SGNN_CHECK_ARG(g.read_ld(o.out) == c.ch(o.out));
  return sgnn_concat3_rows_bwd_dn(g.read(o.out), c.ch(o.in0), c.index(o.ia), c.ch(o.in1), c.index(o.ib), c.ch(o.in2),
                                  c.index(o.ic), c.v.lev_n[o.lev], d[0], o.in0 >= 0 ? c.rows(o.in0) : 0, d[1],
                                  o.in1 >= 0 ? c.rows(o.in1) : 0, d[2], o.in2 >= 0 ? c.rows(o.in2) : 0, c.stream, c.count(o.lev));
}

int bwd_expand(Ctx &c, Grads &g, Lane &lane, int i) {
  const Op &o = c.v.op(i);
  const int in0 = o.in0, cin = o.cin, cout = o.cout;
  const int64_t n = c.v.lev_n[o.lev], ld_nbr = c.v.lev_ld[o.lev], slice = dw_slice(c.v, i);
  const float *dy = g.read(o.out);
  const int32_t *S, *ST, *PAR;
  PROG_TRY(sgnn_expand_maps(&S, &ST, &PAR));
  const float *wc = g.arena + c.L.aux_off[i];
  const int32_t *nbr = (const int32_t *)c.v.lev_nbr[o.lev];
  // reduced 64-slice weight gradient: at the tail of this op's weight-gradient workspace slice (lane-owned memory)
  // (without the lane the slices share `ws` with the BatchNorm kernels: the gradient arena then, as before)
  float *dwc = lane.side ? (float *)(lane.ws + lane.off + slice - expand_dwc_bytes(cin, cout)) : g.garena + c.L.bextra;
  float *part = g.garena + c.L.bextra + round64(64 * (int64_t)cin * cout);
  const hipStream_t ls = lane.fork();
  SGNN_CHECK_ARG(g.read_ld(o.out) == cout && c.ld(in0) == cin);
  if (g.wants(in0) && n > 0) {
    // 64 offsets per parent row, cut into G slices that run as conv groups; the slices are then added
    const int Gs = EXPAND_DX_SPLIT;
    ConvEpi xepi{};
    xepi.n_dev = c.count(o.lev);
    PROG_TRY(sgnn_conv_fwd_impl(dy, 8 * n, cout, wc, 64 / Gs, nbr, ld_nbr, n, cin, part, SGNN_CONV_TRANSPOSE_W, 0, ST, PAR, 8,
                                Gs, 27, &xepi, c.stream));
    float *t = g.target(in0, 0);
    PROG_TRY(sgnn_sum_groups_dn(part, cin, n, Gs, t, c.stream, c.count(o.lev)));
    PROG_TRY(g.commit(in0, t));
  }
  PROG_TRY(sgnn_conv_bwd_weight_impl(g.X(in0), n, cin, cin, dy, cout, cout, nbr, ld_nbr, 8, n, dwc, 0, S, nullptr, 1, 8, 27,
                                     lane.ws + lane.off, slice, (sgnn_stream_t)ls, c.count(o.lev)));
  lane.off += slice;
  lane.pending_expand.push_back(Lane::PendingExpand{dwc, cin, cout, g.PG(o.par)});   // dwc is final after the batched reduce
  return SGNN_OK;
}

int bwd_linear(Ctx &c, Grads &g, Lane &, int i) {
  const Op &o = c.v.op(i);
  const int in0 = o.in0, cin = o.cin, cout = o.cout;
  const int64_t n = c.v.lev_n[o.lev];
  const float *dy = g.read(o.out);
  const float *w[4] = {};
  float *dw[4] = {}, *db[4] = {};
  for (int q = 0; q < cout; ++q) {
    w[q] = c.param(o.par + 2 * q);
    dw[q] = g.PG(o.par + 2 * q);
    db[q] = g.PG(o.par + 2 * q + 1);
  }
  SGNN_CHECK_ARG(g.read_ld(o.out) == cout && c.ld(in0) == cin);
  if (c.P.lin_bn[i] >= 0 && g.wants(in0) && !g.has(in0) && n > 0 && !c.pre[c.P.lin_bn[i]]) {
    // weight / bias gradients only; the BatchNorm before the head forms dx = dy w itself in both of its passes
    PROG_TRY(sgnn_linear_bwd_rows(g.X(in0), dy, n, cin, w, cout, nullptr, dw, db, c.ws, c.ws_bytes, c.stream, c.count(o.lev)));
    g.lazy_lin[in0] = i;
    return SGNN_OK;
  }
  // the input rows already carry a gradient (the caller's, for the rows the next level reads; an alias; or G itself):
  // the head adds it in its own pass — dx = dy w + that — instead of an add launch over the level (round 5)
  const float *have = (g_fuse && g_lin_add && g.wants(in0) && g.has(in0) && n > 0) ? g.read(in0) : nullptr;
  const int64_t have_ld = have ? g.read_ld(in0) : 0;
  if (have && have_ld % 4 == 0 && ((uintptr_t)have & 15) == 0 && !g.viewed[in0]) {
    PROG_TRY(sgnn_linear_bwd_rows(g.X(in0), dy, n, cin, w, cout, g.G(in0), dw, db, c.ws, c.ws_bytes, c.stream, c.count(o.lev),
                                  have, have_ld));
    g.written(in0);
    return SGNN_OK;
  }
  float *t = g.wants(in0) ? g.target(in0, 0) : nullptr;
  PROG_TRY(sgnn_linear_bwd_rows(g.X(in0), dy, n, cin, w, cout, t, dw, db, c.ws, c.ws_bytes, c.stream, c.count(o.lev)));
  return t ? g.commit(in0, t) : SGNN_OK;
}

}  // namespace

// garena has the same layout as arena.  gout[b] != NULL: the caller's gradient of buffer b (a program output); it
// is copied into the arena first (the executor accumulates into its own memory only).  gext[e] != NULL: where the
// gradient of external input e is wanted (fully overwritten).
SGNN_EXPORT int sgnn_prog_backward(const int32_t *ops, const float *opf, int nops, const int32_t *bufs, int nbuf, int n_ext,
                                   const int64_t *lev_n, const int64_t *lev_ld, void *const *lev_nbr,
                                   void *const *lev_children, void *const *lev_ptable, void *const *lev_parent,
                                   void *const *lev_cnt, int nlev, void *const *params,
                                   void *const *pgrads, int nparams,
                                   void *const *ext, void *const *gext, void *const *idx, int nidx,
                                   const float *arena, float *garena, int64_t arena_floats, void *const *gout,
                                   const int32_t *keep, int training, void *ws, int64_t ws_bytes,
                                   sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ops && opf && bufs && lev_n && lev_ld && params && pgrads && arena && garena && gout &&
                 n_ext >= 0 && n_ext <= nbuf && (n_ext == 0 || (ext && gext)));
  Ctx c{View{ops, opf, nops, bufs, nbuf, n_ext, lev_n, lev_ld, lev_nbr, lev_children, lev_ptable, lev_parent, nlev},
        params, idx, lev_cnt, nparams, nidx, training, ws, ws_bytes, stream};
  SGNN_CHECK_ARG(c.prepare(TRAINING, keep));               // the same decisions the forward call took (same inputs)
  if (arena_floats < c.L.total || ws_bytes < ws_need(c.v)) {
    sgnn_set_error("sgnn_prog_backward: arena or workspace too small");
    return SGNN_ENOWS;
  }
  Grads g(c, pgrads, ext, gext, gout, arena, garena);
  PROG_TRY(g.adopt_outputs());
  Lane lane(c, (hipStream_t)stream);
  for (int i = nops - 1; i >= 0; --i) {
    const Op &o = c.v.op(i);
    if (!g.has(o.out) && !(o.type == OP_BN && g.lazy_lin[o.out] >= 0)) {  // no gradient reached this output: its producers contribute nothing
      PROG_TRY(bwd_unreached(c, g, o));
      continue;
    }
    switch (o.type) {
      case OP_CONV_SUBM:
      case OP_CONV_DOWN: PROG_TRY(bwd_conv(c, g, lane, i)); break;
      case OP_UNPOOL: PROG_TRY(bwd_unpool(c, g, lane, i)); break;
      case OP_BN: PROG_TRY(bwd_bn(c, g, lane, i)); break;
      case OP_ADD: PROG_TRY(bwd_add(c, g, lane, i)); break;
      case OP_JOIN: PROG_TRY(bwd_join(c, g, lane, i)); break;
      case OP_CONCAT_IN: PROG_TRY(bwd_concat_in(c, g, lane, i)); break;
      case OP_EXPAND: PROG_TRY(bwd_expand(c, g, lane, i)); break;
      case OP_LINEAR: PROG_TRY(bwd_linear(c, g, lane, i)); break;
      default:
        sgnn_set_error("sgnn_prog_backward: unknown op %d", o.type);
        return SGNN_EINVAL;
    }
  }
  PROG_TRY(g.finish_externals());
  return lane.finish();
}
