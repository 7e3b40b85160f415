import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pocket-tts_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
GOLDEN = ROOT / "tests" / "golden"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP device); parity tests through the C ABI")


def load_golden(name: str) -> dict:
    """A golden fixture; one whose tensors do not fit a 1-MiB file continues in <stem>.part2.safetensors."""
    from safetensors.numpy import load_file

    d = load_file(str(GOLDEN / name))
    part2 = GOLDEN / (Path(name).stem + ".part2.safetensors")
    if part2.exists():
        d.update(load_file(str(part2)))
    return d


def load_ref_wav() -> np.ndarray:
    """The samples of the reference's assets/ref.wav (tests/golden/ref.wav: mono int16, 48 kHz)."""
    import wave

    with wave.open(str(GOLDEN / "ref.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
        return np.frombuffer(w.readframes(w.getnframes()), np.int16)


@pytest.fixture(autouse=True, scope="session")
def _native_build_is_current(request):
    """A GPU session runs only against a library built from these sources (ptts_build_id vs the
    source hash): a stale prebuilt .so pushed to the box fails every GPU test loudly."""
    if any(item.get_closest_marker("gpu") for item in request.session.items):
        import pocket_tts_amd as pt

        pt.check_build_id()


@pytest.fixture(scope="session")
def oracle():
    from _oracle import Oracle

    return Oracle(0x5EED)


@pytest.fixture(scope="session")
def gpu_engine():
    """One 8-slot engine for the GPU parity tests (synthetic weights, seed 0x5EED)."""
    import pocket_tts_amd as pt

    eng = pt.Engine(device=0, max_slots=8, max_ctx=512, lsd_decode_steps=1, seed=0x5EED)
    yield eng
    eng.close()


# fp32 parity gates of the GPU tests (both sides compute in fp32; differences are reduction order
# only). Achieved: latents ~3e-6, PCM ~5e-8 max abs; the golden PCM RMS is 0.035, so PCM_TOL is
# 6e-5 of the signal (north_star's 1e-4 RMS gate is 50x looser).
LAT_TOL = 5e-5  # EOS logit and latent, max abs
PCM_TOL = 2e-6  # PCM, max abs per frame


def pcm_err(a):
    return float(np.abs(np.asarray(a, np.float64)).max())


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))
