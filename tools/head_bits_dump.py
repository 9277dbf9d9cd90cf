#!/usr/bin/env python3
"""Raw output bytes of the SS head, the RSA head and one packed forward, lone and batched, for comparing two builds of the
library bit for bit (lone and packed share their kernels' source, so "packed == lone" inside one build proves less than a
comparison with an earlier build does).

    python tools/head_bits_dump.py OUT_DIR                                   this tree's library
    RNAMSM_LIB_PATH=/path/to/other/librnamsm_hip.so python tools/head_bits_dump.py OTHER_DIR
    diff -r OUT_DIR OTHER_DIR                                                (or cmp file by file)

One file per case, <case>.bin = the float32 outputs as they lie in memory; fixed seeds, the inputs of the tests' truth helpers.
SS (num_blocks = 2, logits and probs): L = 1, 15, 16, 17, 33, 49 lone, then as one batch in that order and reversed.
RSA (K = 3 one-hot, K = 1 embedding only; logits and probs): L = 1, 31, 32, 33, 64, 65, 97 lone, then as one batch in both orders.
Forward: nine alignments of unlike shape through forward_packed (emb and atp of each).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rna-msm_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

DEV = "cuda:0"
SS_LS = [1, 15, 16, 17, 33, 49]
RSA_LS = [1, 31, 32, 33, 64, 65, 97]
FWD_SHAPES = [(1, 21), (5, 133), (16, 40), (17, 33), (3, 9), (33, 64), (2, 257), (4, 12), (7, 16)]


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    from rnamsm import rsa, ss, synthetic
    from rnamsm.model import MSATransformer
    import rsa_truth
    import ss_truth
    count = 0

    def dump(name, t):
        nonlocal count
        t.detach().cpu().numpy().tofile(os.path.join(out_dir, name + ".bin"))
        count += 1

    def both_orders(tag, many, xs, seqs, Ls):
        for order, idx in (("fwd", list(range(len(Ls)))), ("rev", list(reversed(range(len(Ls)))))):
            for i, o in zip(idx, many([xs[i] for i in idx], [seqs[i] for i in idx])):
                dump(f"{tag}_packed_{order}_L{Ls[i]}", o)

    # ---- SS
    head = ss.SSPredictor(2)
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ss_truth.make_state(2, seed=21).items()}, strict=True)
    head = head.eval().to(DEV)
    atps, seqs = [], []
    for i, L in enumerate(SS_LS):
        rng = np.random.RandomState(300 + i)
        a = rng.exponential(size=(120, L, L)).astype(np.float32)
        atps.append(torch.from_numpy(a / a.sum(-1, keepdims=True)).to(DEV))
        seqs.append("".join(rng.choice(list("ACGUN"), L)))
    for want, one, many in (("logits", head.logits, head.logits_many), ("probs", head.predict, head.predict_many)):
        for a, s, L in zip(atps, seqs, SS_LS):
            dump(f"ss_{want}_lone_L{L}", one(a, s))
        both_orders(f"ss_{want}", many, atps, seqs, SS_LS)

    # ---- RSA
    for tag, states, kind in (("rsa3", [rsa_truth.make_state(11 + k) for k in range(3)], "oh"),
                              ("rsa1", [rsa_truth.load_state("state_emb_0")], "emb")):
        st = rsa_truth.load_stats(kind)
        stats = {"emb": (st["emb_mu"], st["emb_std"])}
        if kind == "oh":
            stats["oh"] = (st["oh_mu"], st["oh_std"])
        members = [rsa.RSAPredictor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}) for sd in states]
        ens = rsa.RSAEnsemble(members, stats).eval().to(DEV)
        embs, seqs = [], []
        for i, L in enumerate(RSA_LS):
            rng = np.random.RandomState(500 + i)
            embs.append(torch.from_numpy((st["emb_mu"] + st["emb_std"] * rng.standard_normal((L, 768))).astype(np.float32)).to(DEV))
            seqs.append("".join(rng.choice(list("ACGUN"), L)))
        for want, one, many in (("logits", ens.logits, ens.logits_many), ("probs", ens.predict, ens.predict_many)):
            for e, s, L in zip(embs, seqs, RSA_LS):
                dump(f"{tag}_{want}_lone_L{L}", one(e, s))
            both_orders(f"{tag}_{want}", many, embs, seqs, RSA_LS)

    # ---- one packed forward
    state = synthetic.make_state_dict(seed=0)
    m = MSATransformer(num_layers=10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m = m.eval().to(DEV)
    msas = [torch.from_numpy(synthetic.make_tokens(r, c, 500 + i)).to(DEV) for i, (r, c) in enumerate(FWD_SHAPES)]
    for (r, c), o in zip(FWD_SHAPES, m.forward_packed(msas)):
        dump(f"fwd_packed_emb_{r}x{c}", o["emb"])
        dump(f"fwd_packed_atp_{r}x{c}", o["atp"])
    torch.cuda.synchronize()
    print(f"{count} cases written to {out_dir}")


if __name__ == "__main__":
    main()
