"""fp64 truth for the RNA-MSM-SS head (rnamsm.ss): the reference's network (_downstream_tasks/SS/code/model.py) restated in
torch functional form, at any dtype.  Test infrastructure only: tests/test_ss_truth.py ties it to the reference's own output
(ss_head_b2_l35.npz); the GPU tests then check the HIP head against it at every size."""
import numpy as np
import torch
import torch.nn.functional as F

from rnamsm import ss


def features(atp: np.ndarray, seq: str) -> np.ndarray:
    """[128, L, L]: outer one-hot of the sequence (channels 0-3: base i, 4-7: base j) and the 120 maps."""
    L = atp.shape[-1]
    codes = ss.base_codes(seq)
    oh = np.zeros((L, 4))
    ok = codes < 4
    oh[np.nonzero(ok)[0], codes[ok]] = 1.0
    x = np.zeros((128, L, L))
    x[0:4] = oh.T[:, :, None]
    x[4:8] = oh.T[:, None, :]
    x[8:] = atp
    return x


def make_state(num_blocks: int, seed: int, beta_scale: float = 0.3) -> dict:
    """Random parameters of every kind (LayerNorm affines and both biases included), float32 numpy, reference names."""
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, cout, cin, k):
        sd[name] = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)

    def ln(name):
        sd[name + ".weight"] = (1.0 + 0.3 * rng.standard_normal(48)).astype(np.float32)
        sd[name + ".bias"] = (beta_scale * rng.standard_normal(48)).astype(np.float32)

    conv("conv1.weight", 48, 128, 3)
    sd["conv1.bias"] = (0.3 * rng.standard_normal(48)).astype(np.float32)
    ln("bn1")
    for k in range(num_blocks):
        conv(f"layer1.{k}.conv1.weight", 48, 48, 3)
        ln(f"layer1.{k}.bn1")
        conv(f"layer1.{k}.conv2.weight", 48, 48, 5)
        ln(f"layer1.{k}.bn2")
    sd["fc1.weight"] = (rng.standard_normal((1, 48)) / np.sqrt(48)).astype(np.float32)
    sd["fc1.bias"] = (0.3 * rng.standard_normal(1)).astype(np.float32)
    return sd


def _ln_relu(x, sd, name):
    y = F.layer_norm(x.permute(1, 2, 0), (48,), sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)
    return torch.relu(y.permute(2, 0, 1))


def logits(x: np.ndarray, state: dict, dtype=torch.float64, device="cpu") -> np.ndarray:
    """[L, L] pre-sigmoid output of the head on features x [128, L, L]."""
    sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(device=device, dtype=dtype)
          for k, v in state.items()}
    nb = sum(1 for k in sd if k.endswith(".conv2.weight"))
    h = torch.as_tensor(x).to(device=device, dtype=dtype)[None]
    h = F.conv2d(h, sd["conv1.weight"], sd["conv1.bias"], padding=1)[0]
    for k in range(nb):
        p = f"layer1.{k}"
        t = F.conv2d(_ln_relu(h, sd, p + ".bn1")[None], sd[p + ".conv1.weight"], padding=1)[0]
        h = F.conv2d(_ln_relu(t, sd, p + ".bn2")[None], sd[p + ".conv2.weight"], padding=2)[0] + h
    y = _ln_relu(h, sd, "bn1").permute(1, 2, 0) @ sd["fc1.weight"][0] + sd["fc1.bias"][0]
    return y.cpu().numpy()
