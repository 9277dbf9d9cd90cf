"""likelihood.scan / pseudo_perplexity on the GPU: against the oracle's forward of every masked copy + its LM head, against the old
route (sequence_logits / masked_marginal_scores), across the forward drivers and copies per call, and the token memory it keeps."""
import numpy as np
import pytest
import torch

from oracle import msm_oracle as O
from rnamsm import likelihood, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDX = [1, 4, 11]


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    from rnamsm.model import MSATransformer
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.eval().to(DEV), state


@pytest.fixture(scope="module")
def oracle_5x12(model):
    """Computed once: the oracle's logits at IDX of make_tokens(5, 12, 7), masked copy by masked copy and unmasked."""
    m, state = model
    params = O.to_torch_params(state)
    toks = torch.from_numpy(synthetic.make_tokens(5, 12, 7))
    masked = []
    for i in IDX:
        t = toks.clone()
        t[0, i] = m.vocab.mask_idx
        masked.append(O.lm_head(O.forward(t, params)["representation"][0, i], params))
    plain = O.lm_head(O.forward(toks, params)["representation"][0, IDX], params)
    return toks, torch.stack(masked), plain


def check_scan(s, want_logits: torch.Tensor, wt: torch.Tensor, label: str):
    """The bounds of test_gpu_forward.py::test_masked_pseudo_likelihood_matches_oracle."""
    n = len(wt)
    bound = 1e-4 * max(1.0, float(want_logits.abs().max()))
    err = np.abs(s.logits.cpu().numpy() - want_logits.numpy()).max()
    lp = want_logits.log_softmax(-1)
    ref = lp - lp[torch.arange(n), wt].unsqueeze(1)
    err_sc = np.abs(s.scores.cpu().numpy() - ref.numpy()).max()
    print(f"{label}: logits max-abs {err:.2e} (bound {bound:.2e}), scores max-abs {err_sc:.2e} (bound 2e-4)")
    assert s.logits.shape == s.logp.shape == s.scores.shape == want_logits.shape and s.nll.shape == (n,)
    assert err < bound and err_sc < 2e-4, label
    assert float(s.scores.cpu()[torch.arange(n), wt].abs().max()) == 0.0
    assert torch.equal(s.nll.cpu(), -s.logp.cpu()[torch.arange(n), wt])
    assert np.abs(s.logp.cpu().numpy() - lp.numpy()).max() < 2e-4


def test_scan_matches_the_oracle_and_the_old_route(model, oracle_5x12):
    m, _ = model
    toks, want, plain = oracle_5x12
    wt = toks[0, IDX]
    s = likelihood.scan(m, toks.to(DEV), indices=IDX)
    check_scan(s, want, wt, "scan vs oracle")
    old = likelihood.sequence_logits(m, toks.to(DEV), indices=IDX).cpu()
    check_scan(s, old, wt, "scan vs sequence_logits")
    old_sc = likelihood.masked_marginal_scores(m, toks.to(DEV), indices=IDX).cpu()
    assert np.abs(s.scores.cpu().numpy() - old_sc.numpy()).max() < 2e-4
    # every copies_per_call agrees with every other within the same bounds; the same call twice gives the same bits
    for per in (1, 2, 3):
        again = likelihood.scan(m, toks.to(DEV), indices=IDX, copies_per_call=per)
        check_scan(again, want, wt, f"copies_per_call={per}")
        check_scan(again, s.logits.cpu(), wt, f"copies_per_call={per} vs default")
        twice = likelihood.scan(m, toks.to(DEV), indices=IDX, copies_per_call=per)
        assert all(torch.equal(a, b) for a, b in zip(again, twice))
    # unmasked: one forward, the head on row 0's emb
    check_scan(likelihood.scan(m, toks.to(DEV), indices=IDX, mask_positions=False), plain, wt, "unmasked vs oracle")
    # a one-row alignment given as [C], every column behind <cls> by default
    one = likelihood.scan(m, toks[0].to(DEV), copies_per_call=4)
    assert one.logits.shape == (11, len(m.vocab)) and torch.isfinite(one.scores).all()


def test_the_lone_driver_and_the_batched_driver_agree(model):
    """70 x 64 = 4480 tokens: copies_per_call=1 takes checked_forward_one(need_repr=False) -- the pruned last layer -- and
    copies_per_call=3 the batched driver; three positions only."""
    m, state = model
    toks = torch.from_numpy(synthetic.make_tokens(70, 64, 11))
    idx = [1, 30, 63]
    wt = toks[0, idx]
    lone = likelihood.scan(m, toks.to(DEV), indices=idx, copies_per_call=1)
    batched = likelihood.scan(m, toks.to(DEV), indices=idx, copies_per_call=3)
    check_scan(batched, lone.logits.cpu(), wt, "batched vs lone driver")
    assert all(torch.equal(a, b) for a, b in zip(lone, likelihood.scan(m, toks.to(DEV), indices=idx, copies_per_call=1)))
    params = O.to_torch_params(state)
    t = toks.clone()
    t[0, 30] = m.vocab.mask_idx
    want = O.lm_head(O.forward(t, params)["representation"][0, 30], params)[None]
    check_scan(type(lone)(*(v[1:2] for v in lone)), want, wt[1:2], "lone driver vs oracle, column 30")


def test_pseudo_perplexity_is_the_cross_entropy_of_the_oracle_s_logits(model, oracle_5x12):
    m, _ = model
    toks, want, plain = oracle_5x12
    wt = toks[0, IDX]
    for logits, mask in ((want, True), (plain, False)):
        ce = float(torch.nn.functional.cross_entropy(logits.double(), wt))
        got_log = likelihood.pseudo_perplexity(m, toks.to(DEV), indices=IDX, mask_positions=mask, log=True)
        got = likelihood.pseudo_perplexity(m, toks.to(DEV), indices=IDX, mask_positions=mask)
        print(f"mask={mask}: cross entropy {ce:.6f}, got {got_log:.6f}; perplexity {np.exp(ce):.6f}, got {got:.6f}")
        assert abs(got_log - ce) <= 1e-4 * abs(ce) and abs(got - np.exp(ce)) <= 1e-4 * np.exp(ce)
        assert abs(np.log(got) - got_log) <= 1e-6 * abs(got_log)
    total = likelihood.pseudo_perplexity(m, toks.to(DEV), indices=IDX, reduction="sum", log=True)
    assert abs(total - 3 * float(torch.nn.functional.cross_entropy(want.double(), wt))) <= 3e-4 * abs(total)
    with pytest.raises(ValueError):
        likelihood.pseudo_perplexity(m, toks.to(DEV), indices=IDX, reduction="none")


def test_indices_outside_emb_raise(model):
    m, _ = model
    toks = torch.from_numpy(synthetic.make_tokens(5, 12, 7)).to(DEV)
    for bad in ([0, 3], [12], [3, 12, 4]):
        with pytest.raises(ValueError, match="sequence_logits"):
            likelihood.scan(m, toks, indices=bad)


def test_the_scan_keeps_one_call_s_copies_and_no_more(model):
    """n = 11, copies_per_call = 2 on 32 x 64: the rise of the peak above one forward call of two copies stays within 4 R C 8 bytes
    (the call's own int64 copies are 2 R C 8) plus the outputs -- where mask_and_repeat's [n, R, C] is 11 R C 8."""
    m, _ = model
    R, C, n = 32, 64, 11
    toks = torch.from_numpy(synthetic.make_tokens(R, C, 13)).to(DEV)
    idx = list(range(1, 1 + n))
    likelihood.scan(m, toks, indices=idx[:2], copies_per_call=2)              # the workspace and the weight tables exist from here on
    pair = toks.unsqueeze(0).repeat(2, 1, 1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.checked_forward_batch(pair, False)
    torch.cuda.synchronize()
    one_call = torch.cuda.max_memory_allocated() - base
    del out
    torch.cuda.reset_peak_memory_stats()
    s = likelihood.scan(m, toks, indices=idx, copies_per_call=2)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base - one_call
    calls = -(-n // 2)                                   # the outputs: four per call and their concatenations, in 512-byte blocks
    outputs = calls * 4 * 512 + sum(-(-v.numel() * 4 // 512) * 512 for v in s)
    print(f"one call of two copies {one_call} B; the scan's peak above it {rise} B; bound {4 * R * C * 8 + outputs} B; "
          f"n R C 8 = {n * R * C * 8} B")
    assert rise <= 4 * R * C * 8 + outputs < n * R * C * 8
