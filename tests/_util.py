"""Shared helpers for the tests: golden-fixture loading and comparison utilities."""
import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sub_sd(rec, prefix="sd."):
    """Extract a state_dict (torch tensors, fresh copies) stored under `prefix`."""
    out = {}
    for k, v in rec.items():
        if k.startswith(prefix):
            out[k[len(prefix):]] = torch.from_numpy(np.array(v, copy=True))
    return out


def t(a):
    return torch.from_numpy(np.array(a, copy=True))


def max_abs(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max())


def rel_err(a, b):
    """max|a-b| / max(|b|max, tiny): scale-aware error for gradients."""
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


class kink_matched:
    """Context manager around a HIP forward (+ backward): records the post-ReLU output of every fused conv+ReLU op of
    `model` (engine.RELU_CAPTURE) so that `.masks()` can hand the ReLU masks the kernels actually used to the oracle
    (oracle.ref_cpu.KINK_MASKS).  With matched masks both sides differentiate the same piece of the piecewise-smooth
    network, and the gradient comparison no longer has to tolerate flipped kinks."""

    def __init__(self, model):
        self.model = model
        self.cap = {}

    def __enter__(self):
        import adam_dehaze_amd.engine as E
        self._E = E
        self._old = E.RELU_CAPTURE
        self._old_cbam = E.CBAM_CAPTURE
        E.RELU_CAPTURE = self.cap
        self.cbam = {}
        E.CBAM_CAPTURE = self.cbam
        return self

    def __exit__(self, *exc):
        self._E.RELU_CAPTURE = self._old
        self._E.CBAM_CAPTURE = self._old_cbam
        return False

    def cbam_indices(self):
        """{AttentionBlock 'fc.0.weight' parameter name: (global max-pool arg-max [N, C], per-pixel channel arg-max [N, H*W])} on
        the CPU: the arg-max positions the HIP attention kernels used (the network's other kinks; round 4)."""
        out = {}
        for name, p in self.model.named_parameters():
            o = self.cbam.get(id(p))
            if o is not None:
                out[name] = (o[0].cpu(), o[1].cpu())
        return out

    def post(self):
        """{conv weight parameter name: the post-activation tensor the kernels wrote, [N, >=C, H, W] on the CPU}: what masks()
        is derived from, for kink_audit's gap_dev."""
        out = {}
        for name, p in self.model.named_parameters():
            o = self.cap.get(id(p))
            if o is not None:
                out[name] = o.detach().permute(0, 3, 1, 2).cpu()
        return out

    def masks(self):
        """{conv weight parameter name: bool mask [N, >=C, H, W] on the CPU} (channel padding of the NHWC buffers kept;
        oracle_with_masks crops it)."""
        out = {}
        for name, p in self.model.named_parameters():
            o = self.cap.get(id(p))
            if o is not None:
                out[name] = (o > 0).permute(0, 3, 1, 2).cpu()
        return out


def oracle_with_masks(fn, masks, cbam=None, audit=None):
    """Run `fn()` (an oracle forward + backward) with the ReLUs that follow the listed convolutions forced to `masks` and, given
    `cbam` (kink_matched.cbam_indices()), the attention blocks' arg-max positions forced as well.  `audit`: the KinkAudit of
    these very masks and positions (kink_audit); a forced key it did not audit is an error."""
    from oracle import ref_cpu as R
    if audit is not None:
        audit.covers(masks, cbam)
    old = R.KINK_MASKS
    R.KINK_MASKS = {k: m for k, m in masks.items()}
    old_relu = R._relu
    old_cbam = R.CBAM_INDICES
    R.CBAM_INDICES = cbam

    def _relu(y, key):
        m = masks.get(key)
        if m is None:
            return old_relu(y, key)
        return y * m[:, :y.shape[1]].to(y.dtype)
    R._relu = _relu
    try:
        return fn()
    finally:
        R._relu = old_relu
        R.KINK_MASKS = old
        R.CBAM_INDICES = old_cbam


# ------------------------------------------------------------------------------------------------
# kink audit: is what the tests replay a NEAR-kink?
# ------------------------------------------------------------------------------------------------
class KinkAuditError(AssertionError):
    """the bookkeeping of an audit does not add up (a replayed key that was never visited, never audited, of another shape)"""


class KinkRecord:
    """What a free-running oracle forward took its kinks over, per key and per visit:
      relu[key]  = [pre-activation [N,C,H,W], ...]
      cbam[key]  = [(input of the global max-pool [N,C,H,W], input of the per-pixel channel max [N,C,H,W]), ...]
      pool[key]  = [(pool input [N,C,H,W], kernel, stride), ...]
    Filled by kink_recording(); a test may also build one by hand around a constructed pre-activation."""

    def __init__(self):
        self.relu, self.cbam, self.pool = {}, {}, {}
        self._half = {}


@contextlib.contextmanager
def kink_recording():
    """Records, while a FREE-RUNNING oracle forward runs inside it, every tensor a kink is decided on: the pre-activation of
    every ReLU / ReLU6 (oracle.ref_cpu._relu, tests/_densenet_ref._relu, tests/_mobilenet_ref.RECORD), the two tensors of
    every attention block's maxima (oracle.ref_cpu.KINK_RECORD) and every max-pool input of the loss extractors
    (oracle.ref_cpu._max_pool).  Yields the KinkRecord.  Not to be combined with a replay: an audit compares against what
    the oracle chose on its own."""
    from oracle import ref_cpu as R
    from tests import _densenet_ref as DR
    from tests import _mobilenet_ref as MR
    rec = KinkRecord()
    if R.KINK_MASKS is not None or R.CBAM_INDICES is not None or R.POOL_INDICES is not None:
        raise KinkAuditError("kink_recording() inside a replay: the recorded run has to be free-running")
    old = (R._relu, R._max_pool, R.KINK_RECORD, DR._relu, MR.RECORD)

    def relu(y, key):
        rec.relu.setdefault(key, []).append(y.detach())
        return old[0](y, key)

    def pool(x, k, s, key):
        rec.pool.setdefault(key, []).append((x.detach(), k, s))
        return old[1](x, k, s, key)

    def attention(kind, key, x):
        if kind == "cbam_channel":
            rec._half[key] = x.detach()
        else:
            rec.cbam.setdefault(key, []).append((rec._half.pop(key), x.detach()))

    def dense_relu(y, key, relu_masks):
        if relu_masks is not None:
            raise KinkAuditError("kink_recording() inside a replay: the recorded run has to be free-running")
        rec.relu.setdefault(key, []).append(y.detach())
        return old[3](y, key, relu_masks)

    def mobile(key, z):
        rec.relu.setdefault(key, []).append(z.detach())
    R._relu, R._max_pool, R.KINK_RECORD, DR._relu, MR.RECORD = relu, pool, attention, dense_relu, mobile
    try:
        yield rec
    finally:
        R._relu, R._max_pool, R.KINK_RECORD, DR._relu, MR.RECORD = old


def self_kinks(rec, relu6=False):
    """(masks, post, cbam, pools) a recorded run chose on its own, in the form the tests capture them from the kernels (first
    visit of every key): how the fp32 CPU oracle plays the device in tests/test_kink_audit_cpu.py."""
    masks, post, cbam, pools = {}, {}, {}, {}
    for k, v in rec.relu.items():
        masks[k], post[k] = self_kinks_of(v[0], relu6)
    for k, v in rec.cbam.items():
        x, xc = v[0]
        cbam[k] = (x.flatten(2).argmax(2).to(torch.int32), xc.argmax(1).flatten(1).to(torch.int32))
    for k, v in rec.pool.items():
        x, kk, s = v[0]
        pools[k] = F.max_pool2d(x, kk, s, return_indices=True)[1]
    return masks, post, cbam, pools


# Floors of the audit's magnitude gate, per test family, as a fraction of the audited tensor's float64 max-abs; the gate is
# gap <= 3 * ref + floor (kink_audit).  Each is at most 4 x the worst gap measured in that family on the MI355X and none may
# exceed 1e-4 (KINK_FLOOR_MAX): beyond that an element is not within rounding of its kink and the forward gates of 1e-3
# absolute would not cover it.  They come from the run of every audited test whose per-tensor table is
# profiles/kink_audit.txt (1.7 k tensors; worst gap per family in the comments below).
KINK_FLOOR_MAX = 1e-4
KINK_FLOORS = {
    # the dehazing branches (parity fixtures on three kernel paths, full-width branches on six, joint / branch step, DDP ranks,
    # SSIM): worst 5.8e-6 (medium64, F(4x4,3x3) with the bf16 x 3 contraction; arg-max rows: 5.2e-6); the fp32 CPU oracle: 3.1e-6
    "branches": 2e-5,
    # VGG16 / VGG19 content taps, LPIPS-AlexNet and their single layers, ReLUs and max-pool windows; no BatchNorm, bias-shifted
    # sums of O(1) terms: worst 8.6e-8, five differing elements in all
    "extractors": 3e-7,
    # DenseNet121, train- and eval-mode BatchNorm + ReLU: worst 2.2e-5, ONE element of denseblock4.denselayer15.norm1 at
    # 2 x 70 x 90, where a channel's train-mode statistics come from 8 samples (2 images of 2 x 2 pixels) and the kernels'
    # folded form x * scale + shift (scale = gamma / sigma, shift = beta - mean * scale, both fp32) rounds with |mean| / sigma
    # where F.batch_norm's (x - mean) / sigma does not; the next row is 6.9e-6, the fp32 CPU restatement's worst 4.8e-6
    "densenet": 6e-5,
    # MobileNetV2 (ReLU6, both kinks) / V3 (ReLU, squeeze-excite ReLU): worst 2.2e-5 (features.18.0 of V2, 24 samples per
    # channel, where the fp32 restatement flips the same element: ref 2.2e-5); the worst row with ref ~ 0 is 1.5e-6
    "mobilenet": 2e-5,
}
# where kink_audit() appends its rows: the file ADH_KINK_TABLE names, else the profiling scripts' output directory (git ignores
# it).  profiles/kink_audit.txt is a copy of that file after one run of the whole GPU suite.
KINK_TABLE = os.environ.get("ADH_KINK_TABLE") or os.path.join("profile_out", "kink_audit.txt")


def _relu_row(y, mask, post, relu6):
    """(n_diff, gap64, gap_dev) of one visit, gaps still unscaled.  y: float64 pre-activation, mask / post: what the
    implementation under audit used / wrote there (already cropped to y's shape)."""
    m64 = (y > 0) & (y < 6) if relu6 else y > 0
    diff = mask != m64
    n_diff = int(diff.sum())
    if not n_diff:
        return 0, 0.0, 0.0
    if relu6:      # the kink the element crossed: the nearer one, unless the written value says which side it was put on
        d = torch.minimum(y.abs(), (y - 6).abs())
        d = torch.where(~mask & m64 & (post <= 0), y.abs(), d)
        d = torch.where(~mask & m64 & (post >= 6), (y - 6).abs(), d)
        over = torch.where(y >= 6, 6 - post, post)      # active in the implementation: how far inside the active piece
    else:
        d, over = y.abs(), post
    gap64 = float(d[diff].max())
    on = mask & ~m64
    gap_dev = float(over[on].abs().max()) if bool(on.any()) else 0.0
    return n_diff, gap64, gap_dev


def _choice_row(x, chosen_idx, dim):
    """(n_diff, gap) of an arg-max along `dim` of the float64 tensor x against the indices another implementation chose
    (same shape as x with `dim` of size 1); an index that names a float64 tie of the maximum is the same choice."""
    best = x.max(dim=dim, keepdim=True).values
    got = x.gather(dim, chosen_idx)
    n_diff = int((got != best).sum())
    return n_diff, float((best - got).max()) if got.numel() else 0.0


def _pool_window_check(name, idx, x, k, s):
    Hh, Ww = x.shape[2:]
    OH, OW = idx.shape[2:]
    if int(idx.min()) < 0 or int(idx.max()) >= Hh * Ww:
        raise KinkAuditError(f"{name}: a replayed max-pool index lies outside the {Hh}x{Ww} plane")
    r, c = idx // Ww, idx % Ww
    r0 = (torch.arange(OH) * s).view(1, 1, OH, 1)
    c0 = (torch.arange(OW) * s).view(1, 1, 1, OW)
    if not bool(((r >= r0) & (r < r0 + k) & (c >= c0) & (c < c0 + k)).all()):
        raise KinkAuditError(f"{name}: a replayed max-pool index lies outside its {k}x{k} window")


class KinkAudit:
    """The rows of one kink_audit() call.  covers(): every key a replay forces was audited (oracle_with_masks(audit=...))."""

    def __init__(self, site, path, family):
        self.site, self.path, self.family, self.floor = site, path, family, KINK_FLOORS[family]
        assert self.floor <= KINK_FLOOR_MAX, (family, self.floor)
        self.rows, self.keys = [], set()

    def covers(self, masks=None, cbam=None, pools=None):
        for kind, d in (("relu", masks), ("cbam", cbam), ("pool", pools)):
            missing = sorted(k for k in (d or {}) if (kind, k) not in self.keys)
            if missing:
                raise KinkAuditError(f"{self.site}: replayed but not audited ({kind}): {missing[:6]}")

    def add(self, kind, key, visit, numel, n_diff, scale, gaps, refs):
        self.keys.add((kind, key))
        self.rows.append(dict(kind=kind, key=key, visit=visit, numel=numel, n_diff=n_diff, scale=scale,
                              gaps=[g / scale for g in gaps], refs=[r / scale for r in refs]))

    def lines(self):
        out = []
        for r in self.rows:
            name = f"{r['kind']}:{r['key']}" + (f"#{r['visit']}" if r["visit"] else "")
            g = r["gaps"] + [float("nan")] * (2 - len(r["gaps"]))
            out.append(f"{self.site} | {self.path or '-'} | {name} | numel {r['numel']} | n_diff {r['n_diff']} | gap64 {g[0]:.2e} | "
                       f"gap_dev {g[1]:.2e} | ref {max(r['refs']):.2e} | floor {self.floor:.1e}")
        return out

    def table_lines(self):
        """lines() of the tensors with a differing element, and one line for all the others of this call."""
        rows = list(zip(self.rows, self.lines()))
        same = [r for r, _ in rows if not r["n_diff"]]
        out = [line for r, line in rows if r["n_diff"]]
        if same:
            out.append(f"{self.site} | {self.path or '-'} | {len(same)} other tensor(s) | numel {sum(r['numel'] for r in same)} | n_diff 0 | "
                       f"gaps 0 | ref <= {max(max(r['refs']) for r in same):.2e} | floor {self.floor:.1e}")
        return out

    def failures(self):
        bad = []
        for r, line in zip(self.rows, self.lines()):
            cap = max(8, 1e-3 * r["numel"])
            why = [f"count {r['n_diff']} > {cap:g}"] if r["n_diff"] > cap else []
            why += [f"gap {g:.2e} > 3 * {ref:.2e} + {self.floor:.1e}" for g, ref in zip(r["gaps"], r["refs"])
                    if not g <= 3.0 * ref + self.floor]
            if why:
                bad.append(", ".join(why) + ": " + line)
        return bad

    def worst(self):
        return max([g for r in self.rows for g in r["gaps"]], default=0.0)


def kink_audit(site, rec64, *, family, masks=None, post=None, cbam=None, pools=None, rec32=None, relu6=False, path="",
               gate=True, table=True):
    """Audit what a test is about to replay against what float64 chose on its own.

    rec64: the KinkRecord of the free-running float64 oracle forward (kink_recording()).  masks / cbam / pools: exactly what
    the test hands to the replay (oracle_with_masks, LX.run_forced, relu_masks=, act_masks=), taken from the output under test;
    post {key: post-activation [N, >=C, H, W]}: the tensors the kernels wrote, which the masks came from.  rec32: the
    KinkRecord of the fp32 CPU oracle's free run on the same input: its own choices against rec64 give `ref`, the yardstick
    (0 where it agrees with float64 everywhere).  relu6: True, or a set of keys, for ReLU6 tensors (two kinks).

    Per ReLU tensor and visit (channel padding cropped): n_diff = elements whose replayed mask differs from float64's;
    gap64 = the worst float64 distance of such an element to the kink it crossed; gap_dev = the worst value the kernels wrote
    where they say active and float64 says inactive; both over the tensor's float64 max-abs.  Per attention block, for the
    global max-pool arg-max ("cbam" rows, first) and the per-pixel channel arg-max (second), and per replayed max-pool window:
    n_diff = choices that are not a float64 maximum, gap64 = max64 - x64[replayed index] over the same scale.

    Gate, per row: every gap <= 3 * ref + floor (KINK_FLOORS[family]; the factor 3 as in tests/test_gpu_loss_extractors.py:
    the MFMA kernels' other summation order and F(4x4,3x3) round up to 3 x coarser than the direct sum), and
    n_diff <= max(8, 1e-3 * numel), so that a wholesale error cannot hide as many small ones (one zeroed channel of 96 or
    one row of 64 is >= 1e-2; the fp32 CPU oracle measures <= 1e-5).

    Bookkeeping fails loudly (KinkAuditError): a replayed key the free run never visited, a key without its captured output,
    another shape, an index outside its plane or window.  A key visited several times in one forward (the content loss walks
    its prefix once per tap) is audited per visit, the same replayed mask against each.  The rows go to
    KINK_TABLE before anything is asserted (a tensor without a differing element only as part of a count).  Returns the
    KinkAudit; pass it to oracle_with_masks(audit=...)."""
    masks, cbam, pools, post = masks or {}, cbam or {}, pools or {}, post or {}
    a = KinkAudit(site, path, family)
    is6 = (lambda k: True) if relu6 is True else (lambda k: bool(relu6) and k in relu6)

    def visits(kind, store, key):
        v = store.get(key)
        if not v:
            raise KinkAuditError(f"{site}: replayed {kind} key {key!r} was never visited by the free-running oracle")
        return v

    def crop(what, key, tns, like):
        if tns.dim() != 4 or tns.shape[0] != like.shape[0] or tns.shape[1] < like.shape[1] or tns.shape[2:] != like.shape[2:]:
            raise KinkAuditError(f"{site}: {what} of {key!r} has shape {tuple(tns.shape)}, the oracle's tensor {tuple(like.shape)}")
        return tns[:, :like.shape[1]]

    for key, m in masks.items():
        if key not in post:
            raise KinkAuditError(f"{site}: no captured output for the replayed mask {key!r}")
        v32 = rec32.relu.get(key) if rec32 is not None else None
        for i, y in enumerate(visits("relu", rec64.relu, key)):
            y = y.double()
            mm = crop("mask", key, m.cpu(), y).bool()
            pp = crop("captured output", key, post[key].detach().cpu(), y).double()
            scale = max(float(y.abs().max()), 1e-300)
            n_diff, g64, gdev = _relu_row(y, mm, pp, is6(key))
            refs = (0.0, 0.0)
            if v32 is not None:
                y32 = crop("fp32 oracle tensor", key, v32[i], y)
                m32, p32 = self_kinks_of(y32, is6(key))
                refs = _relu_row(y, m32, p32.double(), is6(key))[1:]
            a.add("relu", key, i, y.numel(), n_diff, scale, (g64, gdev), refs)
    for key, (i0, i1) in cbam.items():
        v32 = rec32.cbam.get(key) if rec32 is not None else None
        for i, (x, xc) in enumerate(visits("cbam", rec64.cbam, key)):
            x, xc = x.double(), xc.double()
            n_, c_, h_, w_ = x.shape
            i0_, i1_ = i0.cpu().to(torch.int64), i1.cpu().to(torch.int64)
            if i0_.numel() != n_ * c_ or i1_.numel() != n_ * h_ * w_:
                raise KinkAuditError(f"{site}: arg-max sets of {key!r} have {i0_.numel()} / {i1_.numel()} entries, the oracle's "
                                     f"tensor is {tuple(x.shape)}")
            if int(i0_.min()) < 0 or int(i0_.max()) >= h_ * w_ or int(i1_.min()) < 0 or int(i1_.max()) >= c_:
                raise KinkAuditError(f"{site}: an arg-max of {key!r} lies outside the tensor")
            for part, tns, idx, dim in (("max-pool", x.flatten(2), i0_.view(n_, c_, 1), 2), ("channel-max", xc, i1_.view(n_, 1, h_, w_), 1)):
                scale = max(float(tns.abs().max()), 1e-300)
                n_diff, gap = _choice_row(tns, idx, dim)
                ref = 0.0
                if v32 is not None:
                    t32 = v32[i][0].flatten(2) if dim == 2 else v32[i][1]
                    ref = _choice_row(tns, t32.argmax(dim, keepdim=True), dim)[1]
                a.add("cbam", f"{key}[{part}]", i, idx.numel(), n_diff, scale, (gap,), (ref,))
            a.keys.add(("cbam", key))
    for key, idx in pools.items():
        v32 = rec32.pool.get(key) if rec32 is not None else None
        for i, (x, k, s) in enumerate(visits("pool", rec64.pool, key)):
            x = x.double()
            idx_ = idx.cpu().to(torch.int64)
            want = F.max_pool2d(x, k, s).shape
            if idx_.shape != want:
                raise KinkAuditError(f"{site}: pool choices of {key!r} have shape {tuple(idx_.shape)}, the oracle's {tuple(want)}")
            _pool_window_check(f"{site}: {key!r}", idx_, x, k, s)
            best = F.max_pool2d(x, k, s).flatten(2)
            got = x.flatten(2).gather(2, idx_.flatten(2))
            scale = max(float(x.abs().max()), 1e-300)
            ref = 0.0
            if v32 is not None:
                i32 = F.max_pool2d(v32[i][0], k, s, return_indices=True)[1]
                ref = float((best - x.flatten(2).gather(2, i32.flatten(2))).max())
            a.add("pool", key, i, idx_.numel(), int((got != best).sum()), scale, (float((best - got).max()),), (ref,))
    a.covers(masks, cbam, pools)
    if table:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(KINK_TABLE)), exist_ok=True)
            with open(KINK_TABLE, "a") as f:
                f.write("\n".join(a.table_lines()) + "\n")
        except OSError:
            if os.environ.get("ADH_KINK_TABLE"):      # a table that was asked for by name has to be writable
                raise
    print(f"[kink audit] {site} {path}: {len(a.rows)} rows, worst gap {a.worst():.2e}, floor {a.floor:.1e}")
    if gate:
        bad = a.failures()
        assert not bad, f"{len(bad)} replayed tensor(s) are not near-kinks:\n" + "\n".join(bad[:8])
    return a


def self_kinks_of(y, relu6):
    """(mask, post-activation) of a pre-activation as a plain implementation in y's own precision decides them."""
    return ((y > 0) & (y < 6), y.clamp(0, 6)) if relu6 else (y > 0, y.clamp_min(0))


# ------------------------------------------------------------------------------------------------
# helpers of the kernel-level GPU tests (test_gpu_train_io / test_gpu_detect_kernels / test_gpu_lpips)
# ------------------------------------------------------------------------------------------------
EPS = 2.0 ** -24            # fp32 unit roundoff
DEV = "cuda:0"


def _nan(*shape, dtype=torch.float32):
    """an output buffer no kernel has written: every element NaN."""
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _idx(*shape):
    """an int32 output buffer no kernel has written: every element -7."""
    return torch.full(shape, -7, device=DEV, dtype=torch.int32)


def _same_bits(u, v):
    if u.is_floating_point():
        it = torch.int64 if u.dtype == torch.float64 else torch.int32
        u, v = u.contiguous().view(it), v.contiguous().view(it)
    return torch.equal(u, v)


def _twice(fn):
    """run fn twice; the two runs' outputs must be bit-equal.  Returns the first run's outputs."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(a, b)):
        assert _same_bits(u, v), f"output {i} differs between two identical runs"
    return a


def _assert_bound(got, ref64, bound, what):
    """|got - ref64| <= bound element-wise (bound: tensor or number); prints the worst ratio before it asserts."""
    assert not torch.isnan(got).any(), f"{what}: NaN (an element was not written)"
    ref64 = torch.as_tensor(ref64, dtype=torch.float64, device=got.device)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device)
    err = (got.double() - ref64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"[bound] {what}: worst |err| / bound = {worst:.3f}")
    d = err - bound
    assert float(d.max()) <= 0, f"{what}: exceeds its bound by {float(d.max()):.3e} (|err| / bound = {worst:.3f})"


def _padded(n, pad=64, dtype=torch.float32, fill=float("nan")):
    """(whole, owned): an allocation of n elements with `pad` guard elements on both sides, all set to `fill`."""
    whole = torch.full((n + 2 * pad,), fill, device=DEV, dtype=dtype)
    return whole, whole[pad:pad + n]


def _pad_untouched(whole, n, pad=64):
    """the guard elements of a _padded allocation still hold their fill (NaN, or -7 for ints)."""
    g = torch.cat([whole[:pad], whole[pad + n:]])
    return bool(torch.isnan(g).all()) if g.is_floating_point() else bool((g == -7).all())
