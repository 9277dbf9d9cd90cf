"""The calls the CLI makes into rnamsm.ops for the two heads, in order: four alignments (one alone, three in a packed group) with
both head keys set and everything else at its default.  The expected list is the trace of the commit before the heads' results
became records (rnamsm.ss.SSResult, rnamsm.rsa.RSAResult), taken with these same wrappers."""
import pytest

from rnamsm import inference, ops
from test_gpu_rsa_head_packed import _model_dir
from test_gpu_ss_pairs import IDS, _run_cli, _square_float_jobs, cli_setup  # noqa: F401  (cli_setup: the fixture)

pytestmark = pytest.mark.gpu

LONE = {"ss_head": lambda atp, *a, **k: atp.shape[-1], "ss_prob_text": lambda p: p.shape[0],
        "ss_pairs": lambda p, l: p.shape[0], "rsa_head": lambda emb, *a, **k: emb.shape[0]}
PACKED = ("ss_head_packed", "ss_prob_text_packed", "ss_pairs_packed", "rsa_head_packed")
EXPECTED = [("ss_head", 100), ("ss_prob_text", 100), ("ss_pairs", 100), ("rsa_head", 100),
            ("ss_head_packed", 3), ("ss_prob_text_packed", 3), ("ss_pairs_packed", 3), ("rsa_head_packed", 3)]


def test_the_eight_head_ops_in_call_order(cli_setup, tmp_path, monkeypatch):
    trace, tensors = [], []

    def wrap(name, size):
        real = getattr(ops, name)

        def counted(*a, **k):
            trace.append((name, size(*a, **k)))
            return real(*a, **k)

        monkeypatch.setattr(ops, name, counted)

    for name, size in LONE.items():
        wrap(name, size)
    for name in PACKED:
        wrap(name, lambda members, *a, **k: len(members))
    real_submit = inference._AsyncNpyWriter.submit

    def submit(self, job_list, done, after=None):
        for _, t in job_list:
            tensors.extend((tuple(x.shape), x.dtype) for x in (t if isinstance(t, tuple) else (t,)))
        return real_submit(self, job_list, done, after=after)

    monkeypatch.setattr(inference._AsyncNpyWriter, "submit", submit)
    files = _run_cli(cli_setup, monkeypatch, "both_heads", [f"data.rsa_model_dir={_model_dir(tmp_path)}"])
    assert trace == EXPECTED
    assert _square_float_jobs(tensors) == [], tensors                          # no [L, L] float copy was handed to the writer
    assert all(files.values())
    res = cli_setup[0] / "both_heads" / "RSA_result"
    assert all((res / f"{i}_{tag}" / f"{i}.txt").stat().st_size for i in IDS for tag in ("0", "1", "2", "ensemble"))
