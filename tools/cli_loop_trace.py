#!/usr/bin/env python3
"""The order of model calls and writer submissions of the CLI loop (rnamsm.inference.extract_feat) on one fixed synthetic list, with the
sha256 of every file written, as JSON on stdout: for an A/B of two commits whose loops must behave alike (profiles/cli_loop_trace_ab.json).  The list: four tiny
alignments that pool, one that is alone in its LayerNorm class (a group of one), two larger lone ones, one containing <pad> and, under
data.long_msa=windows, one just wider than the model (max_seqlen = 65); run once with the heads off and once with data.contacts and
data.lm_scores=wt."""
import contextlib, hashlib, io, json, os, sys, tempfile, shutil
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))
import numpy as np, torch
from rnamsm import inference, synthetic
from rnamsm.config import Config
from rnamsm.model import MSATransformer

MAX_SEQLEN = 65
SHAPES = {"a_tiny0": (3, 20), "b_tiny1": (4, 24), "c_lone0": (300, 60), "d_tiny2": (2, 30), "e_class": (90, 60), "f_pad": (6, 22),
          "g_lone1": (280, 64), "h_tiny3": (5, 18), "i_wide": (4, 70)}
model = MSATransformer(num_layers=10, max_seqlen=MAX_SEQLEN)
model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(seed=0, max_seqlen=MAX_SEQLEN).items()}, strict=True)
trace = []


def shapes_of(x):
    return [list(t.shape) for t in x] if isinstance(x, (list, tuple)) else list(x.shape)


def record(owner, name):
    real = getattr(owner, name)

    def wrapped(self, first, *args, **kwargs):
        trace.append([name, shapes_of(first) if name != "submit" else [os.path.basename(str(p)) if not callable(p) else "<head>" for p, _ in first]]
                     + ([kwargs["what"]] if "what" in kwargs else []))
        return real(self, first, *args, **kwargs)
    setattr(owner, name, wrapped)


for entry in ("forward_one", "finish_forward_one", "checked_forward_one", "forward_ragged", "forward_ragged_begin",
              "forward_ragged_finish", "forward_windows"):
    record(MSATransformer, entry)
record(inference._AsyncNpyWriter, "submit")
real_load = inference.load_msa_tokens


def load_with_pad(path, *args, **kwargs):               # no file holds <pad>: the reader's result gets one
    tokens = real_load(path, *args, **kwargs)
    if "f_pad" in str(path):
        tokens[-1, -1] = 1
    return tokens


inference.load_msa_tokens = load_with_pad
runs = {}
for label, keys in (("heads_off", {}), ("contacts_lm_wt", {"contacts": True, "lm_scores": "wt"})):
    rng = np.random.RandomState(3)
    root = tempfile.mkdtemp(prefix="rnamsm_cli_trace_")
    os.makedirs(os.path.join(root, "results"))
    for name, (depth, length) in SHAPES.items():
        with open(os.path.join(root, "results", f"{name}.a2m_msa2"), "w") as f:
            f.write("".join(f">s{r}\n{''.join(rng.choice(list('ACGU'), length))}\n" for r in range(depth)))
    open(os.path.join(root, "rna_id.txt"), "w").write("\n".join(SHAPES) + "\n")
    cfg = Config()
    cfg.data.root_path, cfg.data.MSA_path, cfg.data.MSA_list = root, "results", "rna_id.txt"
    cfg.data.sample_method, cfg.data.max_seqs_per_msa, cfg.data.max_seqlen, cfg.data.long_msa = "first", 512, MAX_SEQLEN, "windows"
    for k, v in keys.items():
        setattr(cfg.data, k, v)
    del trace[:]
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        written = inference.extract_feat(cfg, model=model)
    runs[label] = {"written": written, "printed": [ln for ln in printed.getvalue().splitlines() if root not in ln],
                   "files": {f: hashlib.sha256(open(os.path.join(root, "results", f), "rb").read()).hexdigest()
                             for f in sorted(os.listdir(os.path.join(root, "results"))) if not f.endswith(".a2m_msa2")}, "trace": [json.dumps(e) for e in trace]}
    shutil.rmtree(root)
print(json.dumps(runs, indent=1))
