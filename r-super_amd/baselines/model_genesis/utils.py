"""Models Genesis pretext pairs on the device (csrc/genesis.hip): generate_one_pair of the reference's baselines/model_genesis/utils.py :206-266 --
per-sample min-max normalisation, flips (:50), local pixel shuffling (:76), the Bezier intensity curve (:61), in-painting (:106) / out-painting (:125)
and the map back to the input range.  The host draws a plan (`plan_genesis_pair`: which transforms fired, the shuffled blocks, the curve's knots, the
painted boxes, one 64-bit seed); the device applies it in at most four launches per eight samples (`generate_pair_batch`, one dispatcher call,
torch.ops.rsuper.genesis_pair).  For the same plan the pair equals the reference's bit for bit (tests/golden/genesis.npz).  No CPU kernel: a CPU
tensor raises RSuperHipError.

Where the draws differ from the reference's: the plan reads numpy's global generator (or a RandomState of its own), not Python's `random`; the
painted noise and -- unless host_permutations=True -- the block permutations come from the device's Philox generator keyed by the plan's seed instead
of np.random.rand / np.random.shuffle.  A device permutation is the stable argsort of one 32-bit key per box voxel: uniform up to the probability of
a tie, about n^2 / 2^33 for a box of n voxels (1.2e-5 for the largest box of a 96^3 crop, 9 x 9 x 9)."""
import numpy as np
import torch

GENESIS_TRANSFORMS = ('flip_d', 'flip_h', 'flip_w', 'shuffle', 'curve', 'inpaint', 'outpaint')    # bit k of a sample's flags
F_SHUFFLE, F_CURVE, F_INPAINT, F_OUTPAINT = 8, 16, 32, 64
MIN_SIDE = 14            # below it the reference's out-painting draws fail (randint over an empty range)
N_KNOTS = 100000         # nTimes of nonlinear_transformation
_BASIS = {}


def _bernstein(n_points, n_times):
    """The (n_points, n_times) Bernstein basis bezier_curve multiplies the control points with; it depends on the two counts alone."""
    key = (n_points, n_times)
    if key not in _BASIS:
        try:
            from scipy.special import comb
        except ImportError:                               # the same values: binomial coefficients of a small n are exact
            from math import comb as _c
            comb = lambda n, i: np.float64(_c(n, i))
        t = np.linspace(0.0, 1.0, n_times)
        n = n_points - 1
        _BASIS[key] = np.array([comb(n, i) * (t ** (n - i)) * (1 - t) ** i for i in range(n_points)])
    return _BASIS[key]


def bezier_curve(points, nTimes=N_KNOTS):
    """bezier_curve (:23-48): the curve of the control points [[x, y], ...] at nTimes parameter values -> (xvals, yvals), float64.  The same
    expression on the same basis, which is kept per (len(points), nTimes): after the first call a curve is two dot products."""
    basis = _bernstein(len(points), nTimes)
    x = np.array([p[0] for p in points])
    y = np.array([p[1] for p in points])
    return np.dot(x, basis), np.dot(y, basis)


class GenesisPlan:
    """Per sample b: flip[b] = the net (D, H, W) flips of x and y; blocks[b] = None or the (nb, 6) int array (z0, y0, x0, nz, ny, nx) of the shuffled
    blocks in the order they apply, perms[b] = None (the device draws them) or one int array of source positions per block; control[b] = None or
    ((x1, y1), (x2, y2), sort_both) and curve[b] = None or the float64 knots (xp, fp) np.interp takes; paint[b] = None, 'in' or 'out' with
    boxes[b] = [(z0, y0, x0, nz, ny, nx), ...]; seed[b] = the 64-bit Philox key of the painted noise and the device permutations."""

    def __init__(self, batch, size):
        self.batch, self.size = batch, tuple(int(s) for s in size)
        self.flip = [(False, False, False)] * batch
        self.blocks, self.perms = [None] * batch, [None] * batch
        self.control, self.curve = [None] * batch, [None] * batch
        self.paint, self.boxes = [None] * batch, [[] for _ in range(batch)]
        self.seed = [0] * batch

    @property
    def flags(self):
        out = []
        for b in range(self.batch):
            f = sum(1 << k for k in range(3) if self.flip[b][k])
            f |= F_SHUFFLE if self.blocks[b] is not None else 0
            f |= F_CURVE if self.curve[b] is not None else 0
            f |= {None: 0, 'in': F_INPAINT, 'out': F_OUTPAINT}[self.paint[b]]
            out.append(f)
        return out

    def fired(self, b):
        return [n for k, n in enumerate(GENESIS_TRANSFORMS) if self.flags[b] >> k & 1]


def _check_size(size):
    size = tuple(int(s) for s in size)
    if len(size) != 3:
        raise ValueError('genesis: size is (D, H, W), got %r' % (size,))
    if min(size) < MIN_SIDE:
        raise ValueError('genesis: every side must be at least %d (the out-painting draws of the reference are empty below), got %r' % (MIN_SIDE, size))
    return size


def _curve_from_control(p1, p2, sort_both, n_knots=N_KNOTS):
    xv, yv = bezier_curve([[0, 0], [p1[0], p1[1]], [p2[0], p2[1]], [1, 1]], nTimes=n_knots)
    return np.sort(xv), (np.sort(yv) if sort_both else yv)


def _per_sample(v, batch, what):
    if v is None:
        return [None] * batch
    v = list(v)
    if len(v) != batch:
        raise ValueError('%s: one value (or None) per sample, got %d for a batch of %d' % (what, len(v), batch))
    return v


def make_genesis_plan(batch, size, flip=None, blocks=None, perms=None, control=None, curve=None, paint=None, boxes=None, seed=None, n_knots=N_KNOTS):
    """A plan from explicit per-sample values: every argument is None or a sequence of `batch` entries, an entry None = that transform did not fire.
    flip: three booleans (D, H, W); blocks: (nb, 6) ints; perms: one sequence of source positions per block (all shuffling samples or none);
    control: ((x1, y1), (x2, y2), sort_both), from which the knots are computed as nonlinear_transformation does, or curve: the knots (xp, fp)
    themselves; paint: 'in' / 'out' with boxes: up to five (z0, y0, x0, nz, ny, nx); n_knots: the curve's nTimes.  Everything is checked against
    `size` here."""
    from ...hip import lib as _l
    size = _check_size(size)
    plan = GenesisPlan(batch, size)
    flip, blocks, perms, control, curve, paint, boxes, seed = (_per_sample(v, batch, n) for v, n in (
        (flip, 'flip'), (blocks, 'blocks'), (perms, 'perms'), (control, 'control'), (curve, 'curve'), (paint, 'paint'), (boxes, 'boxes'), (seed, 'seed')))
    for b in range(batch):
        if flip[b] is not None:
            plan.flip[b] = tuple(bool(f) for f in flip[b])
            if len(plan.flip[b]) != 3:
                raise ValueError('genesis: flip is three booleans (D, H, W)')
        if blocks[b] is not None:
            blk = np.ascontiguousarray(np.asarray(blocks[b], dtype=np.int32).reshape(-1, 6))
            lo, n = blk[:, :3], blk[:, 3:]
            if len(blk) == 0 or (n < 1).any() or (n > _l.GENESIS_MAX_BLOCK_SIDE).any() or (lo < 0).any() or (lo + n > np.array(size)).any():
                raise ValueError('genesis: a shuffled block must lie inside the volume with sides 1 .. %d' % _l.GENESIS_MAX_BLOCK_SIDE)
            plan.blocks[b] = blk
            if perms[b] is not None:
                ps = [np.asarray(p, dtype=np.int32).reshape(-1) for p in perms[b]]
                if len(ps) != len(blk) or any(len(p) != int(np.prod(s)) or not np.array_equal(np.sort(p), np.arange(len(p))) for p, s in zip(ps, n)):
                    raise ValueError('genesis: perms holds one permutation of its box per block')
                plan.perms[b] = ps
        elif perms[b] is not None:
            raise ValueError('genesis: permutations without blocks')
        if control[b] is not None and curve[b] is not None:
            raise ValueError('genesis: give the control points or the knots, not both')
        if control[b] is not None:
            p1, p2, both = control[b]
            plan.control[b] = ((float(p1[0]), float(p1[1])), (float(p2[0]), float(p2[1])), bool(both))
            plan.curve[b] = _curve_from_control(*plan.control[b], n_knots=n_knots)
        if curve[b] is not None:
            xp, fp = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in curve[b])
            if len(xp) != len(fp) or len(xp) < 2 or (np.diff(xp) < 0).any():
                raise ValueError('genesis: the curve is two arrays of at least two knots, xp ascending')
            plan.curve[b] = (xp, fp)
        if paint[b] is not None:
            if paint[b] not in ('in', 'out'):
                raise ValueError("genesis: paint is 'in', 'out' or None")
            bx = [tuple(int(v) for v in q) for q in (boxes[b] or [])]
            if len(bx) > _l.GENESIS_MAX_BOXES or any(len(q) != 6 or min(q[3:]) < 1 or min(q[:3]) < 0 or any(q[j] + q[3 + j] > size[j] for j in range(3))
                                                     for q in bx):
                raise ValueError('genesis: at most %d painted boxes (z0, y0, x0, nz, ny, nx) inside the volume' % _l.GENESIS_MAX_BOXES)
            plan.paint[b], plan.boxes[b] = paint[b], bx
        if seed[b] is not None:
            plan.seed[b] = int(seed[b]) & 0xFFFFFFFFFFFFFFFF
    shuf = [b for b in range(batch) if plan.blocks[b] is not None]
    if len({plan.perms[b] is None for b in shuf}) > 1:
        raise ValueError('genesis: explicit permutations for every shuffling sample of the batch or for none')
    return plan


def plan_genesis_pair(batch, size, flip_rate=0.4, local_rate=0.5, nonlinear_rate=0.9, paint_rate=0.9, inpaint_rate=0.2, num_block=10000, seed=None,
                      host_permutations=False, n_knots=N_KNOTS):
    """The random decisions of generate_one_pair for `batch` samples of `size` = (D, H, W), in the reference's order and with its inclusive ranges,
    from numpy's global generator (seed=None, the convention of plan_intensity_augment) or from np.random.RandomState(seed):
      flips: while random() < flip_rate, at most three times, one of the axes 0, 1, 2 of the reference's (1, D, H, W) sample -- the channel axis
        (nothing moves), D or H; W is never flipped there, and two flips of one axis cancel;
      shuffling: random() < local_rate, then num_block blocks, each side randint(1, side // 10), each corner randint(0, side - block);
      curve: random() < nonlinear_rate, four random() for the two free control points, random() < 0.5 sorts the abscissae only, else both;
      painting: random() < paint_rate, random() < inpaint_rate chooses in-painting: up to five boxes while random() < 0.95, sides
        randint(side // 6, side // 3); else out-painting: one box and up to four more while random() < 0.95, sides side - randint(3 side // 7,
        4 side // 7); corners randint(3, side - box - 3).
    It is not Python's `random` stream, so the values differ from a reference run.  Each sample ends with two 32-bit draws for its seed.
    host_permutations=True also draws the permutations here (rng.permutation per block; exact uniformity, at the cost of uploading them); n_knots: the curve's nTimes (the reference's 100000)."""
    size = _check_size(size)
    rng = np.random if seed is None else np.random.RandomState(seed)
    rint = lambda lo, hi: int(rng.randint(lo, hi + 1))   # inclusive, as random.randint
    cols = {k: [None] * batch for k in ('flip', 'blocks', 'perms', 'control', 'paint', 'boxes', 'seed')}
    for b in range(batch):
        flip, cnt = [False, False, False], 3
        while rng.random() < flip_rate and cnt > 0:
            axis = rint(0, 2)
            if axis > 0:
                flip[axis - 1] = not flip[axis - 1]
            cnt -= 1
        cols['flip'][b] = flip
        if rng.random() < local_rate:
            # the six draws of every block with the reference's ranges, all sides first and then all corners: one generator call each
            sz = np.array(size)
            n = rng.randint(1, sz // 10 + 1, size=(num_block, 3))
            blk = np.concatenate([rng.randint(0, sz - n + 1), n], axis=1).astype(np.int32)
            cols['blocks'][b] = blk
            if host_permutations:
                cols['perms'][b] = [rng.permutation(int(np.prod(q[3:]))) for q in blk]
        if rng.random() < nonlinear_rate:
            p = [float(rng.random()) for _ in range(4)]
            cols['control'][b] = ((p[0], p[1]), (p[2], p[3]), not rng.random() < 0.5)
        if rng.random() < paint_rate:
            corner = lambda n: [rint(3, s - m - 3) for s, m in zip(size, n)]
            boxes = []
            if rng.random() < inpaint_rate:
                cols['paint'][b], cnt = 'in', 5
                while cnt > 0 and rng.random() < 0.95:
                    n = [rint(s // 6, s // 3) for s in size]
                    boxes.append(corner(n) + n)
                    cnt -= 1
            else:
                cols['paint'][b], cnt = 'out', 4
                n = [s - rint(3 * s // 7, 4 * s // 7) for s in size]
                boxes.append(corner(n) + n)
                while cnt > 0 and rng.random() < 0.95:
                    n = [s - rint(3 * s // 7, 4 * s // 7) for s in size]
                    boxes.append(corner(n) + n)
                    cnt -= 1
            cols['boxes'][b] = boxes
        w = rng.randint(0, 1 << 32, size=2, dtype=np.int64)
        cols['seed'][b] = int(w[0]) | (int(w[1]) << 32)
    return make_genesis_plan(batch, size, n_knots=n_knots, **cols)


def _genesis_pair(img, flags, blocks, perm, perm_off, curve, nbox, boxes, seeds, noise=None, workspace=None):
    """The C ABI call.  img (B, 1, D, H, W) f32 on the device; flags / nbox / seeds: B ints, boxes: B * 5 * 6 ints; blocks (B, nb, 6) int32, perm int32
    with perm_off (B, nb) int64, curve (B, 2, n) float64 and noise (img's shape, f32): device tensors or None; workspace: optional uint8 device tensor
    of rsuper_genesis_workspace_bytes bytes -> (x, y), new tensors."""
    import ctypes
    from ...hip import lib as _l
    ts = (img, blocks, perm, perm_off, curve, noise, workspace)
    if any(t is not None and not t.is_cuda for t in ts):
        raise _l.RSuperHipError('genesis_pair needs device tensors (no CPU fallback)')
    if img.dim() != 5 or img.shape[1] != 1 or img.dtype != torch.float32:
        raise ValueError('genesis_pair: image must be float32 (B, 1, D, H, W), got %s %s' % (img.dtype, tuple(img.shape)))
    B, _, D, H, W = img.shape
    nbx = _l.GENESIS_MAX_BOXES
    if len(flags) != B or len(nbox) != B or len(seeds) != B or len(boxes) != B * nbx * 6:
        raise ValueError('genesis_pair: per-sample records do not match the batch of %d' % B)
    nb = n = 0
    if blocks is not None:
        if blocks.dtype != torch.int32 or blocks.dim() != 3 or blocks.shape[0] != B or blocks.shape[2] != 6:
            raise ValueError('genesis_pair: blocks must be int32 (B, nb, 6)')
        blocks, nb = blocks.contiguous(), blocks.shape[1]
    if perm is not None:
        if blocks is None or perm_off is None or perm.dtype != torch.int32 or perm_off.dtype != torch.int64 or tuple(perm_off.shape) != (B, nb):
            raise ValueError('genesis_pair: perm must be int32 with int64 offsets (B, nb) beside blocks')
        perm, perm_off = perm.contiguous(), perm_off.contiguous()
    if curve is not None:
        if curve.dtype != torch.float64 or curve.dim() != 3 or curve.shape[0] != B or curve.shape[1] != 2:
            raise ValueError('genesis_pair: curve must be float64 (B, 2, n)')
        curve, n = curve.contiguous(), curve.shape[2]
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != tuple(img.shape)):
        raise ValueError('genesis_pair: the noise tensor must be float32 of the image shape')
    img = img.contiguous()
    noise = None if noise is None else noise.contiguous()
    L = _l.lib()
    if workspace is None:
        nbytes = L.rsuper_genesis_workspace_bytes(B, D, H, W, nb if any(f & F_SHUFFLE for f in flags) else 0)
        workspace = torch.empty((max(nbytes, 8),), device=img.device, dtype=torch.uint8)
    x, y = torch.empty_like(img), torch.empty_like(img)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(img.device):
        _l.check(L.rsuper_genesis_pair(
            img.data_ptr(), x.data_ptr(), y.data_ptr(), B, D, H, W, (ctypes.c_int * B)(*[int(f) for f in flags]), nb, ptr(blocks), ptr(perm),
            ptr(perm_off), 0 if perm is None else perm.numel(), ptr(curve), n, (ctypes.c_int * B)(*[int(v) for v in nbox]),
            (ctypes.c_int * (B * nbx * 6))(*[int(v) for v in boxes]), (ctypes.c_ulonglong * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]),
            ptr(noise), workspace.data_ptr(), workspace.numel() * workspace.element_size(), torch.cuda.current_stream().cuda_stream), 'genesis_pair')
    return x, y


def genesis_launches(plan):
    """Kernel launches generate_pair_batch makes for this plan."""
    import ctypes
    from ...hip import lib as _l
    return _l.lib().rsuper_genesis_launches(plan.batch, (ctypes.c_int * plan.batch)(*plan.flags))


def _plan_tensors(plan, device):
    """The plan's device arrays: blocks (B, nb, 6) padded with empty records (which the device skips), the concatenated permutations with their
    offsets, the knots (B, 2, n) -- or None where nothing of the batch needs them."""
    B = plan.batch
    blocks = perm = perm_off = curve = None
    shuf = [b for b in range(B) if plan.blocks[b] is not None]
    if shuf:
        nb = max(len(plan.blocks[b]) for b in shuf)
        blk = np.zeros((B, nb, 6), np.int32)
        for b in shuf:
            blk[b, :len(plan.blocks[b])] = plan.blocks[b]
        blocks = torch.from_numpy(blk).to(device)
        if plan.perms[shuf[0]] is not None:
            off = np.zeros((B, nb), np.int64)
            parts, at = [], 0
            for b in shuf:
                lens = np.array([len(p) for p in plan.perms[b]], np.int64)
                off[b, :len(lens)] = at + np.concatenate([[0], np.cumsum(lens)[:-1]])
                parts += plan.perms[b]
                at += int(lens.sum())
            perm, perm_off = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(device), torch.from_numpy(off).to(device)
    curved = [b for b in range(B) if plan.curve[b] is not None]
    if curved:
        n = len(plan.curve[curved[0]][0])
        if any(len(plan.curve[b][0]) != n for b in curved):
            raise ValueError('genesis: the curves of one batch must have the same number of knots')
        cv = np.zeros((B, 2, n), np.float64)
        for b in curved:
            cv[b, 0], cv[b, 1] = plan.curve[b]
        curve = torch.from_numpy(cv).to(device)
    return blocks, perm, perm_off, curve


def generate_pair_batch(img, plan=None, noise=None, **rates):
    """The pretext pair of a batch of volumes (B, 1, D, H, W) f32 on the device, each sample with its own draws: `plan` (default:
    plan_genesis_pair(B, (D, H, W), **rates), drawn here) says what fires; noise: optional explicit field of the painted values (the image's shape,
    the frame of the result) instead of the in-kernel one.  One dispatcher call, torch.ops.rsuper.genesis_pair -> (x, y), new tensors: x the
    transformed input of the network, y its target, both in the value range of img."""
    from ...hip import lib as _l
    from ...hip import ops as _ops          # noqa: F401  (hip/ops.py pulls in hip/library.py; this order avoids the import cycle)
    from ...hip import library as _library
    if not img.is_cuda or (noise is not None and not noise.is_cuda):
        raise _l.RSuperHipError('genesis_pair needs device tensors (no CPU fallback)')
    if img.dim() != 5 or img.shape[1] != 1 or img.dtype != torch.float32:
        raise ValueError('genesis_pair: image must be float32 (B, 1, D, H, W), got %s %s' % (img.dtype, tuple(img.shape)))
    if max(img.shape[2:]) > _l.GENESIS_MAX_AXIS:
        raise _l.RSuperHipError('genesis_pair failed: RSUPER_ERR_ARG (an axis above %d: a shuffled block side would pass %d)'
                                % (_l.GENESIS_MAX_AXIS, _l.GENESIS_MAX_BLOCK_SIDE))
    if plan is None:
        plan = plan_genesis_pair(img.shape[0], img.shape[2:], **rates)
    elif rates:
        raise ValueError('generate_pair_batch: rates are for drawing a plan; one was given')
    if plan.batch != img.shape[0] or tuple(plan.size) != tuple(img.shape[2:]):
        raise ValueError('generate_pair_batch: the plan is for %d samples of %r, the batch is %r' % (plan.batch, plan.size, tuple(img.shape)))
    blocks, perm, perm_off, curve = _plan_tensors(plan, img.device)
    nbx = _l.GENESIS_MAX_BOXES
    boxes = []
    for b in range(plan.batch):
        flat = [v for q in plan.boxes[b] for v in q]
        boxes += flat + [0] * (nbx * 6 - len(flat))
    seeds = [s - (1 << 64) if s >= (1 << 63) else s for s in plan.seed]        # the schema's ints are signed 64-bit
    x, y = _library.install_genesis_ops(_genesis_pair)(img, plan.flags, blocks, perm, perm_off, curve, [len(q) for q in plan.boxes], boxes, seeds,
                                                      noise, None)
    return x, y


def generate_one_pair(img, flip_rate=0.4, local_rate=0.5, nonlinear_rate=0.9, paint_rate=0.9, inpaint_rate=0.2):
    """generate_one_pair (:206-266) for a device tensor: (D, H, W), (1, D, H, W) or (B, 1, D, H, W) float32 -> (x, y) of the same rank."""
    if img.dim() not in (3, 4, 5):
        raise ValueError('generate_one_pair: a volume of rank 3, 4 or 5, got rank %d' % img.dim())
    v = img.reshape((1,) * (5 - img.dim()) + tuple(img.shape))
    if v.shape[1] != 1:
        raise ValueError('generate_one_pair: one channel, got %d' % v.shape[1])
    x, y = generate_pair_batch(v.float(), flip_rate=flip_rate, local_rate=local_rate, nonlinear_rate=nonlinear_rate, paint_rate=paint_rate,
                               inpaint_rate=inpaint_rate)
    return x.reshape(img.shape), y.reshape(img.shape)
