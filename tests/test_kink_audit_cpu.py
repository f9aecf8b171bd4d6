"""The kink audit (tests/_util.py: kink_recording / kink_audit) on the CPU: the fp32 CPU oracle plays the device.  Its own
ReLU masks, attention arg-max positions and pool choices must pass against the free-running float64 oracle; every planted
fault -- planted in the audit's INPUTS, nothing that runs is changed -- must be rejected with a message that names the
tensor; and the magnitude gate must tell a flip just under the floor from one at ten times the floor."""
import pytest
import torch

from oracle import ref_cpu as R
from tests import _loss_extractor as LX
from tests import _mobilenet_ref as MR
from tests._thirdparty_init import lpips_alex_sd
from tests._util import (KINK_FLOOR_MAX, KINK_FLOORS, KinkAuditError, KinkRecord, kink_audit, kink_recording, load_golden,
                         oracle_with_masks, self_kinks, sub_sd, t)

ORACLE_FWD = {"light_b8": R.lightweight_forward, "lowint_b8": R.low_intensity_forward, "medium_b8": R.medium_forward,
              "medium_b8_odd": R.medium_forward, "corun_b8": R.corun_forward, "high_b16": R.high_forward,
              "high_b16_odd": R.high_forward, "dual_b16": R.dual_branch_forward}
FLOOR = KINK_FLOORS["branches"]


def _record(fwd, x, sd, dtype):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad(), kink_recording() as rec:
        fwd(x.to(dtype), sd, training=True)
    return rec


_cache = {}


def _fixture(name):
    """(rec64, rec32, (masks, post, cbam, pools) of the fp32 run) of a branch fixture; computed once, never modified."""
    if name not in _cache:
        g = load_golden(name)
        rec64 = _record(ORACLE_FWD[name], t(g["x"]), sub_sd(g), torch.float64)
        rec32 = _record(ORACLE_FWD[name], t(g["x"]), sub_sd(g), torch.float32)
        _cache[name] = (rec64, rec32, self_kinks(rec32))
    return _cache[name]


def test_floors_respect_the_hard_limit():
    assert KINK_FLOORS and all(0 < f <= KINK_FLOOR_MAX for f in KINK_FLOORS.values()) and KINK_FLOOR_MAX == 1e-4


@pytest.mark.parametrize("name", sorted(ORACLE_FWD))
def test_genuine_masks_of_the_fp32_oracle_pass(name):
    rec64, rec32, (masks, post, cbam, _) = _fixture(name)
    assert len(masks) >= 5 and set(masks) == set(rec64.relu)
    if name.startswith(("high", "dual")):
        assert cbam
    a = kink_audit(f"cpu {name}", rec64, family="branches", masks=masks, post=post, cbam=cbam, rec32=rec32, table=False)
    assert len(a.rows) == len(masks) + 2 * len(cbam)
    # against itself as the yardstick every row sits at gap == ref; without a yardstick the floor alone has to carry it
    assert all(r["gaps"] == r["refs"] for r in a.rows)
    assert sum(r["n_diff"] for r in a.rows) <= 8
    kink_audit(f"cpu {name}", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)
    oracle_with_masks(lambda: None, masks, cbam, audit=a)


def test_genuine_masks_pass_full_width_light32():
    import adam_dehaze_amd as A
    torch.manual_seed(42)
    sd = {k: v.clone() for k, v in A.LightweightDehazeModel().state_dict().items()}
    hazy, _, _ = R.synthetic_batch(2, 64, 96, seed=42)
    rec64 = _record(R.lightweight_forward, hazy, sd, torch.float64)
    rec32 = _record(R.lightweight_forward, hazy, sd, torch.float32)
    masks, post, _, _ = self_kinks(rec32)
    a = kink_audit("cpu light32", rec64, family="branches", masks=masks, post=post, table=False)
    assert sum(r["numel"] for r in a.rows) > 3_000_000


def test_genuine_relu6_masks_and_pool_choices_pass():
    """ReLU6 (both kinks) on MobileNetV2's restatement, pool windows on LPIPS-AlexNet; and the restatement's forward under
    act_masks keeps its values (6 above the upper kink, not 0): only the derivative is replayed there."""
    name = "mobilenet_v2"
    sd = MR.state_dict(name, seed=4)
    hazy, _, _ = R.synthetic_batch(2, 64, 96, seed=6)
    recs = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad(), kink_recording() as rec:
            out = MR.classifier_forward(hazy.to(dt), LX.cast_sd({k: v.clone() for k, v in sd.items()}, dt), name, training=True)
        recs[dt] = (rec, out)
    rec64, (l64, f64_) = recs[torch.float64]
    masks, post, _, _ = self_kinks(recs[torch.float32][0], relu6=True)
    assert any(bool((p >= 6).any()) for p in post.values()), "the case has saturated channels"
    a = kink_audit("cpu mobilenet_v2", rec64, family="mobilenet", masks=masks, post=post, rec32=recs[torch.float32][0], relu6=True,
                   table=False)
    assert len(a.rows) == len(masks) >= 30
    with torch.no_grad():
        lm, fm = MR.classifier_forward(hazy.double(), LX.cast_sd({k: v.clone() for k, v in sd.items()}, torch.float64), name,
                                       training=True, act_masks=masks)
    assert torch.equal(lm, l64) and torch.equal(fm, f64_)
    # one channel of a ReLU6 tensor left at zero: its mask is false where float64 sits between the kinks
    key = "backbone.features.3.conv.1.0.weight"
    bad_masks, bad_post = dict(masks), dict(post)
    bad_masks[key], bad_post[key] = masks[key].clone(), post[key].clone()
    bad_masks[key][:, 7] = False
    bad_post[key][:, 7] = 0
    with pytest.raises(AssertionError, match="relu:" + key.replace(".", r"\.")):
        kink_audit("cpu mobilenet_v2", rec64, family="mobilenet", masks=bad_masks, post=bad_post, relu6=True, table=False)

    sd = lpips_alex_sd(5)
    x = torch.rand(2, 3, 35, 47, generator=torch.Generator().manual_seed(1))
    recs = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad(), kink_recording() as rec:
            LX.alex_features(x.to(dt), LX.cast_sd(sd, dt))
        recs.append(rec)
    masks, post, _, pools = self_kinks(recs[1])
    assert len(masks) == 5 and len(pools) == 2
    a = kink_audit("cpu lpips", recs[0], family="extractors", masks=masks, post=post, pools=pools, rec32=recs[1], table=False)
    assert len(a.rows) == 7
    key = "loss_fn.net.2"
    moved = dict(pools)
    moved[key] = pools[key].clone()
    moved[key][0, 0, 0, 0] = 4 * recs[0].pool[key][0][0].shape[3] + 4      # pixel (4, 4): outside window (0, 0)
    with pytest.raises(KinkAuditError, match="outside its 3x3 window"):
        kink_audit("cpu lpips", recs[0], family="extractors", masks=masks, post=post, pools=moved, table=False)
    x0 = recs[0].pool[key][0][0]
    spread = x0[1, :, 0:3, 0:3].flatten(1)
    c = int((spread.max(1).values - spread.min(1).values).argmax())      # the channel whose first window is least flat
    lo = int(spread[c].argmin())
    assert float(spread[c].max() - spread[c].min()) > 1e-2 * float(x0.abs().max())
    moved[key] = pools[key].clone()
    moved[key][1, c, 0, 0] = (lo // 3) * x0.shape[3] + lo % 3
    with pytest.raises(AssertionError, match=r"pool:loss_fn\.net\.2"):
        kink_audit("cpu lpips", recs[0], family="extractors", masks=masks, post=post, pools=moved, table=False)


def test_a_key_visited_once_per_tap_is_audited_per_visit():
    from tests._thirdparty_init import vgg16_sd
    sd = vgg16_sd(2)
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    recs = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad(), kink_recording() as rec:
            R.content_loss(x.to(dt), (1 - x).to(dt), LX.cast_sd(sd, dt), taps=(9, 16))
        recs.append(rec)
    assert len(recs[0].relu["model.0.weight"]) == 2 and len(recs[0].relu["model.10.weight"]) == 1
    masks, post, _, pools = self_kinks(recs[1])
    pred = {k: v for k, v in masks.items() if not k.startswith(R.TARGET_KINKS)}
    ppools = {k: v for k, v in pools.items() if not k.startswith(R.TARGET_KINKS)}
    a = kink_audit("cpu content", recs[0], family="extractors", masks=pred, post=post, pools=ppools, rec32=recs[1], table=False)
    assert sum(1 for r in a.rows if r["key"] == "model.0.weight") == 2
    assert any("#1" in line for line in a.lines())


# ------------------------------------------------------------------------------------------------ planted faults (high_b16)
KEY = "encoder.0.1.conv1.block.0.weight"        # a 32-channel ReLU at half resolution
CBAM_KEY = "encoder.0.3.fc.0.weight"


def _plant(fault):
    rec64, _, (masks, post, cbam, _) = _fixture("high_b16")
    masks, post, cbam = dict(masks), dict(post), dict(cbam)
    m = masks[KEY].clone()
    if fault == "channel":
        m[:, 5] = False
    elif fault == "tile":
        m[0, :, 4:8, 4:8] = False
    elif fault == "last-row":
        m[:, :, -1] = False
    elif fault == "shifted":
        m = torch.roll(m, 1, dims=3)
    elif fault == "all-true":
        m[:] = True
    masks[KEY] = m
    post[KEY] = post[KEY] * m        # what a kernel with that fault would have written
    return rec64, masks, post, cbam


@pytest.mark.parametrize("fault", ["channel", "tile", "last-row", "shifted", "all-true"])
def test_planted_mask_fault_is_rejected_by_name(fault):
    rec64, masks, post, cbam = _plant(fault)
    y = rec64.relu[KEY][0]
    assert int((masks[KEY] != (y > 0)).sum()) >= 16
    with pytest.raises(AssertionError, match="relu:" + KEY.replace(".", r"\.")) as e:
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)
    assert not isinstance(e.value, KinkAuditError)
    assert str(e.value).startswith("1 replayed tensor"), "and no other tensor is blamed"


def test_planted_spatial_argmax_moved_to_a_clearly_lower_neighbour():
    rec64, masks, post, cbam = _plant(None)
    x = rec64.cbam[CBAM_KEY][0][0]
    n_, c_, h_, w_ = x.shape
    scale = float(x.abs().max())
    idx = cbam[CBAM_KEY][0].clone().to(torch.int64)
    for c in range(c_):       # a channel whose right-hand (or left-hand) neighbour of the maximum is clearly lower
        p = int(idx[0, c])
        q = p + 1 if p % w_ < w_ - 1 else p - 1
        if float(x[0, c].flatten()[p] - x[0, c].flatten()[q]) > 1e-2 * scale:
            idx[0, c] = q
            break
    else:
        pytest.fail("no channel with a clear maximum")
    cbam[CBAM_KEY] = (idx.to(torch.int32), cbam[CBAM_KEY][1])
    with pytest.raises(AssertionError, match=r"cbam:encoder\.0\.3\.fc\.0\.weight\[max-pool\]"):
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)


def test_planted_channel_argmax_replaced_by_a_fixed_channel():
    rec64, masks, post, cbam = _plant(None)
    xc = rec64.cbam[CBAM_KEY][0][1]
    n_, c_, h_, w_ = xc.shape
    lowest = xc[0].flatten(1).min(0)
    drop = xc[0].flatten(1).max(0).values - lowest.values
    pix = int(drop.argmax())      # ONE pixel, given the channel that is lowest there
    assert float(drop[pix]) > 1e-2 * float(xc.abs().max())
    idx = cbam[CBAM_KEY][1].clone()
    idx.view(n_, h_ * w_)[0, pix] = int(lowest.indices[pix])
    cbam[CBAM_KEY] = (cbam[CBAM_KEY][0], idx)
    with pytest.raises(AssertionError, match=r"cbam:encoder\.0\.3\.fc\.0\.weight\[channel-max\]"):
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)


def test_replayed_key_the_oracle_never_visits_is_an_error():
    rec64, masks, post, cbam = _plant(None)
    masks["decoder.7.block.0.weight"] = masks[KEY]
    post["decoder.7.block.0.weight"] = post[KEY]
    with pytest.raises(KinkAuditError, match=r"decoder\.7\.block\.0\.weight.*never visited"):
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)
    cbam["bottleneck.9.fc.0.weight"] = cbam[CBAM_KEY]
    del masks["decoder.7.block.0.weight"]
    with pytest.raises(KinkAuditError, match=r"bottleneck\.9\.fc\.0\.weight.*never visited"):
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, cbam=cbam, table=False)


def test_replayed_key_missing_from_the_audit_is_an_error():
    rec64, masks, post, cbam = _plant(None)
    fewer = {k: v for k, v in masks.items() if k != KEY}
    a = kink_audit("cpu planted", rec64, family="branches", masks=fewer, post=post, table=False)
    with pytest.raises(KinkAuditError, match="not audited.*" + KEY.replace(".", r"\.")):
        oracle_with_masks(lambda: None, masks, audit=a)
    with pytest.raises(KinkAuditError, match=r"not audited \(cbam\)"):
        oracle_with_masks(lambda: None, fewer, cbam, audit=a)
    del post[KEY]
    with pytest.raises(KinkAuditError, match="no captured output"):
        kink_audit("cpu planted", rec64, family="branches", masks=masks, post=post, table=False)


def test_recording_refuses_a_replayed_run():
    rec64, masks, post, cbam = _plant(None)

    def run():
        with kink_recording():
            pass
    with pytest.raises(KinkAuditError, match="free-running"):
        oracle_with_masks(run, masks, cbam)


# ------------------------------------------------------------------------------------------------ the thresholds discriminate
@pytest.mark.parametrize("relu6", [False, True])
@pytest.mark.parametrize("side", ["dev-active", "dev-inactive"])
def test_single_flip_just_under_the_floor_passes_and_at_ten_floors_fails(side, relu6):
    """A constructed pre-activation of scale 4 (8 under ReLU6, so that the upper kink is inside): one element at distance d
    from a kink, on float64's inactive side with the implementation calling it active (it wrote d / 2), or the other way
    round.  d = 0.9 floor passes, d = 10 floors fails, on gap64; a written value of 10 floors alone fails on gap_dev."""
    g = torch.Generator().manual_seed(9)
    scale = 8.0 if relu6 else 4.0
    base = (torch.rand(1, 4, 6, 6, generator=g, dtype=torch.float64) * 2 + 1) * torch.where(
        torch.rand(1, 4, 6, 6, generator=g) < 0.5, -1.0, 1.0)      # 1 <= |y| <= 3: nothing else near a kink
    base[0, 0, 0, 0] = scale
    base[0, 1, 0, 0] = -scale / 2
    kink = 6.0 if relu6 else 0.0
    outward = 1.0 if relu6 else -1.0      # the direction from the kink into float64's inactive piece

    def audit(d, written=None):
        y = base.clone()
        y[0, 2, 3, 3] = kink + (outward if side == "dev-active" else -outward) * d * scale
        rec = KinkRecord()
        rec.relu["k"] = [y]
        mask = (y > 0) & (y < 6) if relu6 else y > 0
        post = y.clamp(0, 6) if relu6 else y.clamp_min(0)
        mask[0, 2, 3, 3] = side == "dev-active"
        inside = kink - outward * (d * scale / 2 if written is None else written * scale)
        post[0, 2, 3, 3] = inside if side == "dev-active" else kink
        return kink_audit("cpu threshold", rec, family="branches", masks={"k": mask}, post={"k": post}, relu6=relu6, table=False)
    a = audit(0.9 * FLOOR)
    assert a.rows[0]["n_diff"] == 1 and a.rows[0]["gaps"][0] == pytest.approx(0.9 * FLOOR, rel=1e-6)
    with pytest.raises(AssertionError, match="relu:k"):
        audit(10 * FLOOR)
    if side == "dev-active":
        assert audit(0.9 * FLOOR, written=0.9 * FLOOR).rows[0]["gaps"][1] == pytest.approx(0.9 * FLOOR, rel=1e-6)
        with pytest.raises(AssertionError, match="relu:k"):
            audit(0.9 * FLOOR, written=10 * FLOOR)


def test_count_cap_catches_many_small_flips():
    """2000 elements of 1e6 within a tenth of the floor of zero, all called active: every gap is fine, the count is not."""
    g = torch.Generator().manual_seed(4)
    y = torch.rand(1, 10, 100, 1000, generator=g, dtype=torch.float64) + 0.5
    y.view(-1)[:2000] = -0.1 * FLOOR
    rec = KinkRecord()
    rec.relu["k"] = [y]
    post = y.clamp_min(0)
    post.view(-1)[:2000] = 0.05 * FLOOR
    with pytest.raises(AssertionError, match="count 2000 > 1000"):
        kink_audit("cpu count", rec, family="branches", masks={"k": torch.ones_like(y, dtype=torch.bool)}, post={"k": post},
                   table=False)
    y.view(-1)[1000:2000] = 0.5
    post.view(-1)[1000:2000] = 0.5
    kink_audit("cpu count", rec, family="branches", masks={"k": torch.ones_like(y, dtype=torch.bool)}, post={"k": post}, table=False)
