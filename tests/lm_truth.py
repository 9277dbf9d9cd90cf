"""Truth for the LM head on chosen rows (rnamsm.lm / rnamsm_lm_head): oracle.msm_oracle.lm_head plus the log-softmax, the scores and
the nll of utils/likelihood.py, restated at any dtype on given feature rows -- fp64 is the truth, fp32 the yardstick of the GPU
tests' bars (tests/ss_truth.py: compare).  Test infrastructure only."""
import numpy as np
import torch

from oracle import msm_oracle as O

NAMES = ("dense.weight", "dense.bias", "layer_norm.weight", "layer_norm.bias", "weight", "bias")     # rnamsm._lib.W_LM


def head_state(D: int, V: int, seed: int, proj_scale: float = 1.0) -> dict:
    """Random LM-head parameters of every kind (the LayerNorm affine and both biases included), float32 numpy, under the
    checkpoint's names; for D = 768, V = 12 use synthetic.make_state_dict's instead (state_of)."""
    rng = np.random.RandomState(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)        # noqa: E731
    return {"lm_head.dense.weight": f(rng.standard_normal((D, D)) / np.sqrt(D)),
            "lm_head.dense.bias": f(0.3 * rng.standard_normal(D)),
            "lm_head.layer_norm.weight": f(1.0 + 0.3 * rng.standard_normal(D)),
            "lm_head.layer_norm.bias": f(0.3 * rng.standard_normal(D)),
            "lm_head.weight": f(proj_scale * rng.standard_normal((V, D)) / np.sqrt(D)),
            "lm_head.bias": f(0.3 * rng.standard_normal(V))}


def state_of(full: dict, proj_scale: float = 1.0) -> dict:
    """The LM head's six entries of a whole state_dict (synthetic.make_state_dict), the projection scaled."""
    sd = {"lm_head." + n: np.asarray(full["lm_head." + n], dtype=np.float32) for n in NAMES}
    sd["lm_head.weight"] = (sd["lm_head.weight"] * np.float32(proj_scale)).astype(np.float32)
    return sd


def head(x, state: dict, wt=None, dtype=torch.float64) -> dict:
    """{logits, logp [n, V]; with wt also scores [n, V], nll [n]} of the feature rows x [n, D] as numpy arrays of `dtype`.  A wt
    outside [0, V) gives a NaN row of scores and nll."""
    params = O.to_torch_params(state, dtype=dtype)
    feats = torch.as_tensor(np.asarray(x)).to(dtype)
    logits = O.lm_head(feats, params)
    logp = logits.log_softmax(-1)
    out = {"logits": logits, "logp": logp}
    if wt is not None:
        w = torch.as_tensor(np.asarray(wt)).long()
        ok = (w >= 0) & (w < logits.shape[-1])
        ref = logp[torch.arange(len(w)), torch.where(ok, w, torch.zeros_like(w))]
        ref = torch.where(ok, ref, torch.full_like(ref, float("nan")))
        out["scores"] = logp - ref[:, None]
        out["nll"] = -ref
    return {k: v.numpy() for k, v in out.items()}
