"""The programs test_gpu_prog_fp64.py runs through the native executor and test_prog_ref.py through the fp64 interpreter
alone: small hand-built op lists (Net), their sites, data and the plan each is meant to take.

Integer cases (SUBM, DOWN, UNPOOL, ADD, JOIN, CONCAT_IN, EXPAND only; data and weights in {-1, 0, 1}, weights and output
gradients thinned out so that every sum of |terms| stays below 2^24) are compared bit for bit; real cases (anything with
BatchNorm or a head) against the bars of test_gpu_prog_fp64.py.  Seeds of the real cases are chosen so that no BatchNorm
pre-activation of the fp64 reference lies near zero (test_prog_ref.py asserts it).

test_gpu_prog_bf16.py runs the same cases through the bf16 executor: there the integer cases are the exact ones (every
stored value is a bf16 value, test_prog_ref.py asserts it under the data of data(geom, bf16=True))."""
import numpy as np
import torch

OP_SUBM, OP_DOWN, OP_UNPOOL, OP_BN, OP_ADD, OP_JOIN, OP_CONCAT_IN, OP_EXPAND, OP_LINEAR = range(9)
OPW = 12
# externals of the exact cases under the bf16 data: 1 + 2^-8 lies halfway between the bf16 values 1 and 1 + 2^-7 and
# rounds to the even one, 1; a sum of three unrounded ones, 3 + 3 x 2^-8, rounds to 3 + 2^-6 and gives a reader away
# that took the fp32 tensor where it should have taken the bf16 copy
BF16_EXT_SCALE = 1.0 + 2.0 ** -8


class Net(object):
    """Raw op-list builder with the conventions of sgnn_amd.scn.program.Program: rows classes 0..nlev-1 are the pyramid,
    named classes ('child' = 8 x level 0, source classes) follow; parameter slots in op order."""

    def __init__(self):
        self.ops, self.opf, self.bufs, self.slots, self.classes = [], [], [], [], []
        self.n_ext = 0

    def _cls(self, lev):
        if isinstance(lev, str):
            if lev not in self.classes:
                self.classes.append(lev)
            return -1 - self.classes.index(lev)
        return lev

    def _new(self, lev, ch):
        self.bufs.append([self._cls(lev), ch])
        return len(self.bufs) - 1

    def _slot(self, *entries):
        first = len(self.slots)
        self.slots.extend(entries)
        return first

    def _emit(self, t, in0=-1, in1=-1, out=-1, par=-1, lev=0, cin=0, cout=0, in2=-1, ia=-1, ib=-1, ic=-1, opf=(0, 0, 0, 0)):
        self.ops.append([t, in0, in1, out, par, lev, cin, cout, in2, ia, ib, ic])
        self.opf.append(list(opf))
        return len(self.ops) - 1

    def lev(self, b):
        return self.bufs[b][0]

    def ch(self, b):
        return self.bufs[b][1]

    def ext(self, lev, ch):
        assert not self.ops and self.n_ext == len(self.bufs)
        self.n_ext += 1
        return self._new(lev, ch)

    def subm(self, x, cout):
        b = self._new(self.lev(x), cout)
        self._emit(OP_SUBM, x, -1, b, self._slot(('w', (27, self.ch(x), cout))), self.lev(x), self.ch(x), cout)
        return b

    def down(self, x, cout):
        b = self._new(self.lev(x) + 1, cout)
        self._emit(OP_DOWN, x, -1, b, self._slot(('w', (8, self.ch(x), cout))), self.lev(x), self.ch(x), cout)
        return b

    def unpool(self, x):
        b = self._new(self.lev(x) - 1, self.ch(x))
        self._emit(OP_UNPOOL, x, -1, b, -1, self.lev(x) - 1, self.ch(x), self.ch(x))
        return b

    def bn(self, x, leak=0.0):
        c = self.ch(x)
        b = self._new(self.lev(x), c)
        s = self._slot(('gamma', (c,)), ('beta', (c,)), ('rm', (c,)), ('rv', (c,)))
        self._emit(OP_BN, x, -1, b, s, self.lev(x), c, c, opf=(1e-4, 0.9, leak, 0))
        return b

    def add(self, a, c):
        b = self._new(self.lev(a), self.ch(a))
        self._emit(OP_ADD, a, c, b, -1, self.lev(a), self.ch(a), self.ch(a))
        return b

    def join(self, a, c):
        b = self._new(self.lev(a), self.ch(a) + self.ch(c))
        self._emit(OP_JOIN, a, c, b, -1, self.lev(a), self.ch(a), self.ch(c))
        return b

    def concat_in(self, srcs, slots):
        """srcs: three external buffers or None; slots: their index-array slots or None."""
        ins = [-1 if s is None else s for s in srcs]
        ids = [-1 if s is None else s for s in slots]
        b = self._new(0, sum(self.ch(s) for s in srcs if s is not None))
        self._emit(OP_CONCAT_IN, ins[0], ins[1], b, -1, 0, 0, 0, ins[2], ids[0], ids[1], ids[2])
        return b

    def expand(self, x, cout):
        b = self._new('child', cout)
        self._emit(OP_EXPAND, x, -1, b, self._slot(('w', (27, self.ch(x), cout))), 0, self.ch(x), cout)
        return b

    def linear(self, x, nout):
        b = self._new(self.lev(x), nout)
        s = self._slot(*[e for _ in range(nout) for e in (('lw', (1, self.ch(x))), ('lb', (1,)))])
        self._emit(OP_LINEAR, x, -1, b, s, self.lev(x), self.ch(x), nout)
        return b

    def finish(self):
        self.nlev = 1 + max([b[0] for b in self.bufs if b[0] >= 0] + [o[5] + (1 if o[0] in (OP_DOWN, OP_UNPOOL) else 0)
                                                                    for o in self.ops if o[5] >= 0] + [0])
        for b in self.bufs:
            if b[0] < 0:
                b[0] = self.nlev + (-1 - b[0])
        for o in self.ops:
            if o[5] < 0:
                o[5] = self.nlev + (-1 - o[5])
        self.class_ids = dict((name, self.nlev + k) for k, name in enumerate(self.classes))
        self.n_classes = self.nlev + len(self.classes)
        self.ops_np = np.ascontiguousarray(np.array(self.ops, dtype=np.int32).reshape(-1, OPW))
        self.opf_np = np.ascontiguousarray(np.array(self.opf, dtype=np.float32).reshape(-1, 4))
        self.bufs_np = np.ascontiguousarray(np.array(self.bufs, dtype=np.int32).reshape(-1, 2))
        self.n_idx = 1 + max([max(o[9:12]) for o in self.ops] + [-1])
        return self


class Case(object):
    """net: a finished Net; keep / gout: buffers the caller reads / feeds gradients into; gext_null: externals whose
    gradient is not wanted; plan: what sgnn_prog_plan must report with the fusions on, {'add_dst': {op: v}, 'join_view':
    {op: v}, 'lin_bn': {op: v}, 'root' / 'col' / 'ld': {buffer: v}} (what is not listed: add_dst / lin_bn -1, join_view 0,
    every buffer its own root at column 0 with ld = channels); zero_slots: parameter slots whose gradient must be exactly
    zero; extra_rows: rows of the named source classes.  bf16_density: the weight density of an integer case's data for
    the bf16 executor (data(geom, bf16=True)); the plan of the bf16 layout follows from `plan` (expected_plan)."""

    def __init__(self, name, net, integer, keep, gout, plan, side=16, occupancy=0.3, seed=0, gext_null=(), zero_slots=(),
                 extra_rows=None, knobs=None, empty=False, bf16_density=0.25):
        self.name, self.net, self.integer, self.keep, self.gout, self.plan = name, net, integer, list(keep), list(gout), plan
        self.side, self.occupancy, self.seed = side, occupancy, seed
        self.gext_null, self.zero_slots, self.extra_rows = list(gext_null), list(zero_slots), dict(extra_rows or {})
        self.knobs, self.empty, self.bf16_density = knobs, empty, bf16_density

    def coords(self):
        """Level-0 sites [z, y, x, b] of one batch entry inside side^3 (side even at every pyramid level)."""
        if self.empty:
            return np.zeros((0, 4), dtype=np.int64)
        rng = np.random.default_rng(1000 + self.seed)
        s = self.side
        assert s % (1 << (self.net.nlev - 1)) == 0
        cells = np.nonzero(rng.random(s ** 3) < self.occupancy)[0]
        cells = rng.permutation(cells)
        return np.stack([cells // (s * s), (cells // s) % s, cells % s, np.zeros_like(cells)], 1).astype(np.int64)

    def rows(self, geom):
        net = self.net
        r = [0] * net.n_classes
        for l in range(net.nlev):
            r[l] = geom.n[l]
        for name, cid in net.class_ids.items():
            r[cid] = 8 * geom.n[0] if name == 'child' else self.extra_rows[name]
        return r

    def data(self, geom, bf16=False):
        """(params, ext, idx, gouts) as CPU fp32 tensors, from the case's seed alone.  bf16: the data of the bf16 executor's
        test, which differs for integer cases only: their weights are thinned out to bf16_density, so that every value
        the program stores is exactly a bf16 value (test_prog_ref.py), and their externals are +-BF16_EXT_SCALE instead
        of +-1: fp32 values that are no bf16 values and that the executor must round (to +-1) before use."""
        net = self.net
        rows = self.rows(geom)
        gen = torch.Generator().manual_seed(77 + self.seed)

        def ints(shape, density):
            v = torch.randint(-1, 2, tuple(shape), generator=gen).float()
            return v * (torch.rand(tuple(shape), generator=gen) < density).float()

        params = []
        for kind, shape in net.slots:
            if self.integer:
                assert kind == 'w'
                params.append(ints(shape, self.bf16_density if bf16 else 0.25))
            elif kind == 'w':
                params.append(torch.randn(shape, generator=gen) * (2.0 / (shape[0] * shape[1])) ** 0.5)
            elif kind == 'gamma':
                params.append(0.5 + torch.rand(shape, generator=gen))
            elif kind == 'rv':
                params.append(0.5 + torch.rand(shape, generator=gen))
            elif kind == 'lw':
                params.append(torch.randn(shape, generator=gen) * shape[1] ** -0.5)
            else:               # beta, rm, lb
                params.append(torch.randn(shape, generator=gen) * 0.3)
        ext = []
        for b in range(net.n_ext):
            shape = (rows[net.bufs[b][0]], net.bufs[b][1])
            ext.append(ints(shape, 1.0) if self.integer else torch.randn(shape, generator=gen))
            if self.integer and bf16:
                ext[-1] = ext[-1] * BF16_EXT_SCALE
        idx = []
        for s in range(net.n_idx):
            src = [o[1 + k] if k < 2 else o[8] for o in net.ops if o[0] == OP_CONCAT_IN for k in range(3) if o[9 + k] == s]
            n_src = rows[net.bufs[src[0]][0]]
            # unique indices (the contract of the row kernels: no two sites share a source row), the other sites get -1
            m = min(n_src, int(0.8 * rows[0]))
            j = torch.full((rows[0],), -1, dtype=torch.int32)
            j[torch.randperm(rows[0], generator=gen)[:m]] = torch.randperm(n_src, generator=gen)[:m].int()
            idx.append(j)
        gouts = {}
        for b in self.gout:
            shape = (rows[net.bufs[b][0]], net.bufs[b][1])
            gouts[b] = ints(shape, 0.25) if self.integer else torch.randn(shape, generator=gen)
        return params, ext, idx, gouts


def _residual(name, c, d, bn, seed=0, knobs=None):
    n = Net()
    x = n.ext(0, c)
    h = n.subm(x, d)
    if bn:
        h = n.bn(h)
    h2 = n.subm(h, c)
    y = n.add(x, h2)
    n.finish()
    from_conv = len(n.ops) - 2
    fused = (d, c) in ((16, 16), (12, 8))
    return Case(name, n, not bn, [y], [y], {'add_dst': {from_conv: y if fused else -1}}, seed=seed, knobs=knobs)


def _self_add():
    n = Net()
    x = n.ext(0, 8)
    h = n.subm(x, 8)
    y = n.add(h, h)
    n.finish()
    return Case('self_add', n, True, [y], [y], {'add_dst': {0: -1}})


def _join(name, c, c0, c1, bn, seed=0, knobs=None):
    """[conv or BN | UnPooling] producers written in place into the join; gout on the join buffer itself (a viewed
    buffer: its gradient is copied into the arena) and on the convolution behind it."""
    n = Net()
    x = n.ext(0, c)
    a = n.subm(x, c0)
    if bn:
        a = n.bn(a)
    d = n.down(x, c1)
    if bn:
        d = n.bn(d)
    u = n.unpool(d)
    j = n.join(a, u)
    z = n.subm(j, 8)
    n.finish()
    jop = len(n.ops) - 2
    return Case(name, n, not bn, [j, z], [j, z],
                {'join_view': {jop: 1}, 'root': {a: j, u: j}, 'col': {u: c0}, 'ld': {a: c0 + c1, u: c0 + c1}}, seed=seed,
                knobs=knobs)


def _join_col(name, c0, bn, second='conv', seed=0, bf16_density=0.25):
    """An in-place JoinTable whose second input starts at column c0 = 6, 10 or 12: in bf16 rows that is byte 12, 20 or 24
    (= 12, 4, 8 mod 16), where a view is aligned to a dword or to 8 bytes only (join_int_8_12 reaches byte 16).  The
    integer form writes there from a convolution epilogue, the BatchNorm form from BatchNorm's apply pass or, with
    second = 'unpool', from the UnPooling gather."""
    n = Net()
    x = n.ext(0, 8)
    a = n.bn(n.subm(x, c0)) if bn else n.unpool(n.down(x, c0))
    if second == 'unpool':
        b = n.unpool(n.bn(n.down(x, 12)))
    else:
        b = n.subm(x, 12)
        if bn:
            b = n.bn(b)
    j = n.join(a, b)
    z = n.subm(j, 8)
    n.finish()
    jop = len(n.ops) - 2
    return Case(name, n, not bn, [j, z], [j, z],
                {'join_view': {jop: 1}, 'root': {a: j, b: j}, 'col': {b: c0}, 'ld': {a: c0 + 12, b: c0 + 12}}, seed=seed,
                bf16_density=bf16_density)


def _nested_6_12(name, bn, seed=0, bf16_density=0.25):
    """[[6 | 12] | 8]: the inner JoinTable is in place (second input at column 6), the outer one copies (a storage root is
    never itself a view, see _nested_joins) and so puts its second input at column 6 + 12 = 18 of 26-channel rows — byte
    36 of a bf16 row."""
    n = Net()
    x = n.ext(0, 8)
    if bn:
        a, b, c = n.bn(n.subm(x, 6)), n.unpool(n.bn(n.down(x, 12))), n.bn(n.subm(x, 8))
    else:
        a, b, c = n.unpool(n.down(x, 6)), n.subm(x, 12), n.subm(x, 8)
    j1 = n.join(a, b)
    j2 = n.join(j1, c)
    z = n.subm(j2, 8)
    n.finish()
    jop = len(n.ops) - 3
    return Case(name, n, not bn, [z], [z], {'join_view': {jop: 1, jop + 1: 0}, 'root': {a: j1, b: j1}, 'col': {b: 6},
                                             'ld': {a: 18, b: 18}}, seed=seed, bf16_density=bf16_density)


def _two_joins():
    n = Net()
    x = n.ext(0, 8)
    a, b, c = n.subm(x, 8), n.subm(x, 8), n.subm(x, 8)
    j1 = n.join(a, b)
    j2 = n.join(a, c)
    y = n.add(j1, j2)
    n.finish()
    return Case('two_joins_read_one_buffer', n, True, [y], [y], {'join_view': {3: 0, 4: 0}})


def _join_ext_kept():
    n = Net()
    x = n.ext(0, 8)
    a = n.subm(x, 8)
    j = n.join(x, a)            # an external side: no view
    b = n.subm(j, 8)            # kept below: no view
    c = n.subm(j, 12)
    j2 = n.join(b, c)
    n.finish()
    return Case('join_of_external_and_kept', n, True, [b, j2], [b, j2], {'join_view': {1: 0, 4: 0}})


def _nested_joins():
    """One JoinTable's output is another's input.  The inner join is in place; the outer one copies, because make_plan
    accepts only convolution, BatchNorm and UnPooling producers for an in-place input and the producer of j1 is a
    JoinTable: a storage root is therefore never itself a view."""
    n = Net()
    x = n.ext(0, 8)
    a, b, c = n.subm(x, 8), n.subm(x, 8), n.subm(x, 12)
    j1 = n.join(a, b)
    j2 = n.join(j1, c)
    z = n.subm(j2, 8)
    n.finish()
    return Case('nested_joins', n, True, [z], [z], {'join_view': {3: 1, 4: 0}, 'root': {a: j1, b: j1}, 'col': {b: 8},
                                                     'ld': {a: 16, b: 16}})


def _two_readers():
    n = Net()
    x = n.ext(0, 8)
    h = n.subm(x, 8)
    p = n.subm(h, 8)
    q = n.subm(h, 8)
    s = n.add(p, q)             # fused into q's epilogue
    t = n.add(s, h)
    y = n.add(t, h)             # h: two aliased contributions (materialised), then two convolutions add in place
    n.finish()
    return Case('two_readers', n, True, [y], [y], {'add_dst': {2: s}})


def _u3(name='u3', seed=0, knobs=None, keep_mid=False, empty=False):
    n = Net()
    x = n.ext(0, 8)
    a = n.bn(n.subm(x, 8))
    b = n.bn(n.subm(n.down(a, 12), 12))
    c = n.bn(n.subm(n.down(b, 16), 16))
    u2 = n.unpool(c)
    j1 = n.join(b, u2)
    e = n.bn(n.subm(j1, 16))
    u1 = n.unpool(e)
    j0 = n.join(a, u1)
    z = n.subm(j0, 16)
    n.finish()
    t = [o[0] for o in n.ops]
    jops = [i for i, v in enumerate(t) if v == OP_JOIN]
    plan = {'join_view': {jops[0]: 1, jops[1]: 1}, 'root': {b: j1, u2: j1, a: j0, u1: j0}, 'col': {u2: 12, u1: 8},
            'ld': {b: 28, u2: 28, a: 24, u1: 24}}
    keep, gout = [z], [z]
    if keep_mid:                # an intermediate output with a gradient of its own: c is kept, e is kept
        keep, gout = [z, c, e], [z, c, e]
    return Case(name, n, False, keep, gout, {} if empty else plan, side=16, occupancy=0.35, seed=seed, knobs=knobs, empty=empty)


def _no_gout(seed=0):
    n = Net()
    x = n.ext(0, 8)
    a = n.subm(x, 8)
    b = n.bn(n.subm(x, 8))
    l = n.linear(b, 1)
    n.finish()
    return Case('output_without_gradient', n, False, [a, l], [a], {'lin_bn': {3: 2}}, zero_slots=[1, 2, 3, 6, 7], seed=seed)


def _stage(name, kept_bn, none_source, gext_null=(), integer=False, seed=0, skip_rows=420, empty=False):
    """CONCAT_IN of three sources -> convolution -> [BatchNorm] -> 8-child up-sampling convolution -> [BatchNorm -> two
    heads].  The integer variant stops behind the up-sampling convolution."""
    n = Net()
    s0 = n.ext('prev', 8)
    s1 = None if none_source else n.ext('prev', 2)
    s2 = n.ext('skip', 8 if none_source else 6)
    cat = n.concat_in([s0, s1, s2], [0, None if none_source else 0, 1])
    h = n.subm(cat, 16)
    if integer:
        e = n.expand(h, 8)
        n.finish()
        return Case(name, n, True, [e], [e], {}, side=8, occupancy=0.5, seed=seed, gext_null=gext_null,
                    extra_rows={'prev': 150, 'skip': 220})
    h = n.bn(h)
    e = n.expand(h, 8)
    f = n.bn(e)
    y = n.linear(f, 2)
    n.finish()
    lop, bop = len(n.ops) - 1, len(n.ops) - 2
    keep = [y, f] if kept_bn else [y]
    return Case(name, n, False, keep, keep, {'lin_bn': {lop: -1 if kept_bn else bop}}, side=8, occupancy=0.7, seed=seed,
                gext_null=gext_null, extra_rows={'prev': 300, 'skip': skip_rows}, empty=empty)


def _single_ops():
    out = []
    for name, build in (('subm', lambda n, x: n.subm(x, 8)), ('down', lambda n, x: n.down(x, 12)),
                        ('unpool', lambda n, x: n.unpool(n.down(x, 8))), ('add', lambda n, x: n.add(x, n.subm(x, 8))),
                        ('join', lambda n, x: n.join(x, n.subm(x, 12))), ('expand', lambda n, x: n.expand(x, 8))):
        n = Net()
        y = build(n, n.ext(0, 8))
        n.finish()
        plan = {'add_dst': {0: y}} if name == 'add' else {}
        out.append(Case('op_' + name, n, True, [y], [y], plan, side=8 if name == "expand" else 16,
                        occupancy=0.5 if name == 'expand' else 0.3))
    n = Net()
    n.bn(n.ext(0, 12))
    n.finish()
    out.append(Case('op_bn', n, False, [1], [1], {}, seed=0))
    n = Net()
    n.linear(n.ext(0, 16), 2)
    n.finish()
    out.append(Case('op_linear', n, False, [1], [1], {}))
    n = Net()
    a, b = n.ext('prev', 5), n.ext('skip', 3)
    n.concat_in([a, None, b], [0, None, 1])
    n.finish()
    out.append(Case('op_concat_in', n, True, [2], [2], {}, extra_rows={'prev': 300, 'skip': 200}))
    return out


TILE = {'conv_small': 0}
WIDE = {'conv_small_rows': 0, 'conv_wide_epi': 1, 'conv_unrolled': 1}

# seeds of the real cases: the first of 0, 1, 2, ... that passes the ReLU guard (test_prog_ref.py)
SEEDS = {'u3': 3, 'u3_kept_middle': 3, 'stage_lin_add': 1, 'output_without_gradient': 2, 'join_bn_5_8': 2,
         'join_bn_12_12': 3}


def cases():
    s = lambda name: SEEDS.get(name, 0)
    out = _single_ops()
    out += [_residual('residual_int_8_12', 8, 12, False), _residual('residual_int_5_7', 5, 7, False), _self_add(),
            _join('join_int_8_12', 8, 8, 12, False), _nested_joins(), _two_joins(), _join_ext_kept(), _two_readers(),
            _stage('stage_int', False, False, integer=True)]
    for name, c, d in (('residual_16_16', 16, 16), ('residual_8_12', 8, 12), ('residual_5_7', 5, 7)):
        out.append(_residual(name, c, d, True, s(name)))
    out.append(_join('join_bn_5_7', 5, 5, 7, True, s('join_bn_5_7')))
    # 8 un-pooled channels at column 5 of 13-float rows: a stride that is no multiple of 4 forces the scalar form of the
    # strided gather and of its gradient's gather-sum on a width that would otherwise take float4
    out.append(_join('join_bn_5_8', 8, 5, 8, True, s('join_bn_5_8')))
    # in-place joins at the columns a bf16 view can get wrong
    out += [_join_col('join_int_6_12', 6, False), _join_col('join_int_10_12', 10, False), _join_col('join_int_12_12', 12, False),
            _nested_6_12('nested_int_6_12_8', False)]
    out += [_join_col('join_bn_6_12', 6, True, seed=s('join_bn_6_12')),
            _join_col('join_bn_10_12', 10, True, 'unpool', seed=s('join_bn_10_12')),
            _join_col('join_bn_12_12', 12, True, seed=s('join_bn_12_12')),
            _nested_6_12('nested_bn_6_12_8', True, seed=s('nested_bn_6_12_8'))]
    out.append(_u3('u3', s('u3')))
    out.append(_u3('u3_kept_middle', s('u3_kept_middle'), keep_mid=True))
    out.append(_no_gout(s('output_without_gradient')))
    out.append(_stage('stage_lin_bn', False, False, seed=s('stage_lin_bn')))
    out.append(_stage('stage_lin_add', True, True, seed=s('stage_lin_add')))
    out.append(_stage('stage_gext_null', False, False, gext_null=[1], seed=s('stage_gext_null')))
    # empty rows classes: every level empty (no launch may fail, every gradient is zero), a source without rows
    out.append(_u3('u3_all_levels_empty', empty=True))
    out.append(_stage('stage_level0_empty', False, False, empty=True))
    out.append(_stage('stage_empty_source', False, False, seed=s('stage_empty_source'), skip_rows=0))
    # kernel families: the same programs with the tile kernels' strided epilogues forced at these small sizes
    out.append(_residual('residual_8_12_tile64', 8, 12, True, s('residual_8_12'), TILE))
    out.append(_residual('residual_8_12_wide', 8, 12, True, s('residual_8_12'), WIDE))
    out.append(_u3('u3_tile64', s('u3'), TILE))
    out.append(_u3('u3_wide', s('u3'), WIDE))
    return out


def case_names():
    return [c.name for c in cases()]


def expected_plan(case, fused, bf16=False):
    """Full arrays (skip is implied: fused AddTables and in-place JoinTables) from the case's sparse description.
    bf16: the plan of the bf16 layout (sgnn_prog_plan mode 3) — the same, except that a JoinTable whose first input has an
    odd channel count is not in place, and that every row stride counts bf16 elements and is rounded up to 8 (LINEAR
    outputs stay fp32 rows of their own width)."""
    net = case.net
    nops, nbuf = len(net.ops), len(net.bufs)
    p = case.plan if fused else {}
    want = {'add_dst': [-1] * nops, 'join_view': [0] * nops, 'lin_bn': [-1] * nops, 'root': list(range(nbuf)),
            'col': [0] * nbuf, 'ld': [b[1] for b in net.bufs]}
    for key, d in p.items():
        for k, v in d.items():
            want[key][k] = v
    if bf16:
        for i, o in enumerate(net.ops):
            if want['join_view'][i] and o[6] % 2:
                want['join_view'][i] = 0
                for b in (o[1], o[2]):
                    want['root'][b], want['col'][b] = b, 0
        heads = set(o[3] for o in net.ops if o[0] == OP_LINEAR)
        for b in range(nbuf):
            ch = net.bufs[want['root'][b]][1]
            want['ld'][b] = ch if want['root'][b] in heads else (ch + 7) // 8 * 8
    want['skip'] = [0] * nops
    for i in range(nops):
        if want['join_view'][i] or (i > 0 and want['add_dst'][i - 1] >= 0):
            want['skip'][i] = 1
    return want


def read_plan(lib_query, case, rows, mode=0, keep=None):
    """sgnn_prog_plan for the case's descriptors as a dict of lists (the library's current switches apply); keep: the
    kept buffers, if not the case's own."""
    net = case.net
    nops, nbuf = len(net.ops), len(net.bufs)
    lev_n = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    kept = case.keep if keep is None else list(keep)
    keep = np.zeros(nbuf, dtype=np.int32)
    keep[kept] = 1
    out = np.full(4 * nops + 3 * nbuf, -7, dtype=np.int32)
    rc = lib_query('sgnn_prog_plan', net.ops_np.ctypes.data, nops, net.bufs_np.ctypes.data, nbuf, net.n_ext, lev_n.ctypes.data,
                   net.n_classes, keep.ctypes.data, mode, out.ctypes.data)
    assert rc == 0
    o, b = out[:4 * nops].reshape(nops, 4), out[4 * nops:].reshape(nbuf, 3)
    return {'skip': o[:, 0].tolist(), 'add_dst': o[:, 1].tolist(), 'join_view': o[:, 2].tolist(), 'lin_bn': o[:, 3].tolist(),
            'root': b[:, 0].tolist(), 'col': b[:, 1].tolist(), 'ld': b[:, 2].tolist()}
