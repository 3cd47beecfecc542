"""Every compute call runs on its tensor's device, whichever device is current: the calls that used to launch without a
device guard -- rms_batch and MfccPlan.logmel / stft_power / rfft / modspec / mfcc_change -- give, on tensors of device 1
while device 0 is current, bit for bit what they give with device 1 current.  Needs two visible devices (skipped with
fewer).  The stream read at call time and graph capture are held by tests/test_gpu_streams.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def other():
    """(plan of the default n_fft-512 configuration on device 1, 2 clips of 2048 samples, an MFCC block [2, 13, 64])."""
    import torch
    from modulation_mfcc_amd import MfccConfig, MfccPlan
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    dev = torch.device("cuda", 1)
    rng = np.random.default_rng(7)
    audio = torch.from_numpy(rng.standard_normal((2, 2048)).astype(np.float32)).to(dev)
    mfcc = torch.from_numpy(rng.standard_normal((2, 13, 64)).astype(np.float32)).to(dev)
    cfg = MfccConfig()
    assert cfg.n_fft == 512 and cfg.n_mfcc == 13
    return MfccPlan(cfg, device=dev), audio, mfcc


def _calls(plan, audio, mfcc):
    from modulation_mfcc_amd import butter_sos, rms_batch
    sos = butter_sos(4, 0.2)
    return {
        "rms_batch": lambda: rms_batch(audio, 256, 64),
        "logmel": lambda: plan.logmel(audio),
        "stft_power": lambda: plan.stft_power(audio),
        "rfft": lambda: plan.rfft(audio, 2048),
        "modspec": lambda: plan.modspec(mfcc),
        "mfcc_change": lambda: plan.mfcc_change(mfcc, sos),
    }


def _bits(result):
    import torch
    result = (result,) if isinstance(result, torch.Tensor) else tuple(result)
    torch.cuda.synchronize(result[0].device)
    return [(torch.view_as_real(t) if t.is_complex() else t).cpu().numpy().tobytes() for t in result]


@pytest.mark.parametrize("name", ["rms_batch", "logmel", "stft_power", "rfft", "modspec", "mfcc_change"])
def test_runs_on_the_tensors_device(name, other, gpu):
    import torch
    plan, audio, mfcc = other
    call = _calls(plan, audio, mfcc)[name]
    with torch.cuda.device(0):
        away = call()
        devices = {t.device for t in ((away,) if isinstance(away, torch.Tensor) else away)}
        away = _bits(away)
    with torch.cuda.device(1):
        home = _bits(call())
    assert devices == {audio.device}
    assert away == home
