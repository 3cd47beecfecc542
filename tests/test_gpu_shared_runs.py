"""Shared mel runs in the fused launches of the staged n_fft 512 kernel: every result of a launch on the
shared-runs table is bit for bit the result of the same launch on the overlapping runs (set_shared_runs(False)) -- the
log-mel rows and the clip extremes the launch leaves in the workspace, the MFCC, the modulation spectrum."""
import numpy as np
import pytest
import torch

from modulation_mfcc_amd import MfccConfig, MfccPlan

pytestmark = pytest.mark.gpu

C16K = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
HOP = 160


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32)


def _both(plan, x, modspec=False):
    """{name: tensor} of one call with the shared runs and of the same call with the overlapping ones."""
    res = []
    for shared in (True, False):
        prev = plan.set_shared_runs(shared)
        try:
            assert plan.shared_runs == shared
            if plan._ws is not None:
                plan._ws.fill_(0xA5)
            out = {}
            if modspec:
                out["mfcc"], out["mod"] = plan.mfcc_modspec(x)
            else:
                out["mfcc"] = plan.mfcc(x)
            torch.cuda.synchronize()
            B, n = x.shape
            T = plan.cfg.num_frames(n)
            rows = B * plan.cfg.n_mels * T * 4
            out["logmel"] = plan._ws[:rows].view(torch.float32).clone()
            if not (modspec and plan.fused_tail(B, n)):       # one launch: the extremes never leave the workgroup
                k0 = (rows + 255) // 256 * 256
                out["clip_max_min_keys"] = plan._ws[k0:k0 + 8 * B].view(torch.int32).clone()
            res.append(out)
        finally:
            plan.set_shared_runs(prev)
    return res


def _assert_same(res, what):
    new, old = res
    assert new.keys() == old.keys()
    for k in new:
        assert torch.equal(_bits(new[k]), _bits(old[k])), "%s: %s differs between the two run tables" % (what, k)


def _noise(gpu, B, n, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    t = torch.arange(n, device=gpu, dtype=torch.float32) / 16000.0
    x = 0.05 * torch.randn((B, n), generator=g, device=gpu)
    return x + 0.5 * (1.0 + 0.8 * torch.sin(2 * np.pi * 4.0 * t)) * torch.sin(2 * np.pi * 440.0 * t)


def _burst(gpu, n, seed):
    """silent but for a short burst: the clip clamps, and the fix-up reads the stored rows of every filter"""
    g = torch.Generator(device=gpu).manual_seed(seed)
    x = torch.zeros(n, device=gpu)
    a, b = n // 3, min(n, n // 3 + 200)
    x[a:b] = torch.randn(b - a, generator=g, device=gpu)
    return x


@pytest.fixture(scope="module")
def plan40(gpu):
    plan = MfccPlan(MfccConfig(**C16K))
    assert plan.kernel_path == "radix16-w16s" and plan.fused_dct and plan.shared_runs
    return plan


# frames per clip = 1 + n // hop: 1, 41, 64 (one full tile), 65 (a second tile with one frame), 130 (three tiles)
@pytest.mark.parametrize("frames,batch", [(1, 5), (41, 6), (64, 7), (65, 8), (130, 5)])
def test_mode1_matches_overlapping_runs(plan40, gpu, frames, batch):
    n = 96 if frames == 1 else (frames - 1) * HOP
    assert plan40.cfg.num_frames(n) == frames
    x = _noise(gpu, batch, n, 100 + frames)
    x[batch // 2] = _burst(gpu, n, frames)               # one clip that clamps
    _assert_same(_both(plan40, x), "%d frames x %d clips" % (frames, batch))


def test_mode1_clip_boundary_inside_a_workgroup(plan40, gpu):
    """More tiles than compute units: workgroups walk two or three consecutive tiles, and for many of them the second one
    opens another clip -- the extremes of the finished clip are reduced behind its last tile's finishing step.  Two batch
    sizes, so that both a last tile of one frame (65 frames) and a three-tile clip (130) cross workgroups."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for frames in (65, 130):
        tiles = (frames + 63) // 64
        batch = (2 * cus + cus // 2) // tiles + 1
        assert batch * tiles > 2 * cus
        x = _noise(gpu, batch, (frames - 1) * HOP, 7 + frames)
        x[3] = _burst(gpu, x.shape[1], 11)
        x[batch - 1] = _burst(gpu, x.shape[1], 12)       # the launch's last clip clamps
        _assert_same(_both(plan40, x), "%d clips of %d frames on %d CUs" % (batch, frames, cus))


def test_fewer_tiles_than_workgroups(plan40, gpu):
    x = _noise(gpu, 3, 40 * HOP, 5)
    _assert_same(_both(plan40, x), "3 tiles")


def test_nan_clip_between_finite_ones(plan40, gpu):
    n = 129 * HOP
    x = _noise(gpu, 3, n, 21)
    x[1] = float("nan")
    res = _both(plan40, x)
    _assert_same(res, "NaN clip")
    for out in res:
        assert torch.isfinite(out["mfcc"][0]).all() and torch.isfinite(out["mfcc"][2]).all()


@pytest.mark.parametrize("n_mels", [13, 16])
def test_few_filters(gpu, n_mels):
    """13 mel: parts without a filter are passed over when the hand-over's receiver is looked up; 16 mel: parts of one
    filter, which receive and hand over in their only run."""
    plan = MfccPlan(MfccConfig(**dict(C16K, n_mels=n_mels, n_mfcc=min(13, n_mels))))
    assert plan.kernel_path == "radix16-w16s" and plan.fused_dct and plan.shared_runs
    x = _noise(gpu, 6, 129 * HOP, 31 + n_mels)
    x[4] = _burst(gpu, x.shape[1], 3)
    _assert_same(_both(plan, x), "%d mel" % n_mels)


@pytest.mark.parametrize("name,kw", [("empty filters", None), ("one log-mel tile", dict(C16K, n_mels=89))])
def test_plans_that_keep_the_overlapping_runs(gpu, name, kw):
    plan = MfccPlan(MfccConfig(**kw) if kw else MfccConfig())
    assert plan.kernel_path == "radix16-w16s" and plan.fused_dct
    assert not plan.shared_runs, name
    prev = plan.set_shared_runs(True)
    assert prev is True and not plan.shared_runs, "the switch's default is on; it does not make such a plan share runs"
    x = _noise(gpu, 3, 10244, 41)
    a = plan.mfcc(x).clone()
    plan.set_shared_runs(False)
    assert torch.equal(_bits(a), _bits(plan.mfcc(x)))


@pytest.mark.parametrize("n,n_mod", [(48000, 512), (96000, 1024)])
def test_mode2_matches_overlapping_runs(plan40, gpu, n, n_mod):
    """mfcc_modspec in one launch (clip mode): 256 clips, one of them clamping."""
    B = 256
    assert plan40.cfg.mod_fft_len(plan40.cfg.num_frames(n)) == n_mod
    if B < torch.cuda.get_device_properties(gpu).multi_processor_count:
        B = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert plan40.fused_tail(B, n)
    x = _noise(gpu, B, n, n_mod)
    x[17] = _burst(gpu, n, 9)
    res = _both(plan40, x, modspec=True)
    _assert_same(res, "clip mode, n_mod %d" % n_mod)
    assert torch.isfinite(res[0]["mfcc"]).all() and torch.isfinite(torch.view_as_real(res[0]["mod"])).all()
