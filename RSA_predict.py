#!/usr/bin/env python3
"""Drop-in for the reference's _downstream_tasks/RSA/predict.py (RNA-MSM RSA predictor) on MI355X.

    python RSA_predict.py --rootdir DIR --featdir results --rnaid 2DRB_1 --device cuda

Reads `<featdir>/<rnaid>.fasta` (each record's description is its name) and `<featdir>/<name>_emb.npy` (the [L, 768] embedding
RNA_MSM_Inference.py writes), runs the ensemble of `<rootdir>/models/OH+RNA-MSM_Emb` (model_pcc_*.pt in sorted order and the two
statistic_dict_*.pickle files) on the HIP device (rnamsm.rsa.RSAEnsemble: all members in one set of launches) and writes
`<featdir>/RSA_result/<name>_<k>/<name>.txt` per member and `<featdir>/RSA_result/<name>_ensemble/<name>.txt` as the reference
does.  `random` is seeded with 2022 as there.  --text-device (default): the tables are computed and formatted on the device
(rnamsm_rsa_text) and written as one block each; an embedding of 1025 to 4096 rows, which a stitched long alignment leaves behind,
goes through rnamsm_rsa_head_long / rnamsm_rsa_text_long; --no-text-device: the host arithmetic and np.savetxt, the same bytes.  Not written: the reference's two PNG plots; no device but the HIP one.
"""
import os
import random
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))


def get_args(argv=None):
    p = ArgumentParser()
    p.add_argument("--rootdir", default=ROOT, type=str, help="models at <rootdir>/models/OH+RNA-MSM_Emb")
    p.add_argument("--featdir", default=os.path.join(ROOT, "results"), type=str)
    p.add_argument("--rnaid", default="2DRB_1", type=str)
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the HIP device; there is no CPU path)")
    p.add_argument("--text-device", dest="text_device", action="store_true", default=True,
                   help="format the tables on the device (default); the same bytes as --no-text-device")
    p.add_argument("--no-text-device", dest="text_device", action="store_false", help="format the tables on the host (np.savetxt)")
    return p.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    if not args.device.startswith("cuda"):
        sys.exit(f"RSA_predict.py: --device {args.device}: this build runs on the HIP device only (--device cuda)")
    import numpy as np
    import torch
    from rnamsm import _lib, rsa
    from rnamsm.msa import read_fasta_records

    fasta = os.path.join(args.featdir, args.rnaid + ".fasta")
    model_dir = os.path.join(args.rootdir, "models", "OH+RNA-MSM_Emb")
    if not os.path.isfile(fasta):
        sys.exit(f"RSA_predict.py: {fasta} not found")
    if not os.path.isdir(model_dir):
        sys.exit(f"RSA_predict.py: {model_dir} not found")
    random.seed(2022)
    device = torch.device(args.device)
    ens = rsa.load_ensemble(model_dir, device)
    for name, seq in read_fasta_records(fasta):
        emb_path = os.path.join(args.featdir, name + "_emb.npy")
        if not os.path.isfile(emb_path):
            sys.exit(f"RSA_predict.py: {emb_path} not found")
        emb = np.load(emb_path)
        if emb.ndim != 2 or emb.shape != (len(seq), rsa.EMBED_DIM):
            sys.exit(f"RSA_predict.py: {name}: sequence of length {len(seq)} but an embedding of shape {emb.shape} in {emb_path}")
        with torch.no_grad():
            emb_dev = torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float32)).to(device)
            # an embedding of more than 1024 rows (a stitched long alignment's, data.long_msa=windows) takes the long entry points
            long_ = emb.shape[0] > _lib.RSA_MAX_L
            if args.text_device:
                values, text = (ens.predict_text_long if long_ else ens.predict_text)(emb_dev, seq)
                text = tuple(t.cpu().numpy() for t in text)
            else:
                values, text = (ens.predict_long if long_ else ens.predict)(emb_dev, seq), None
        rsa.write_rsa_files(values.cpu().numpy(), seq, name, args.featdir, ens.model_names, random, text=text)
        print(f"{name}: {os.path.join(args.featdir, 'RSA_result', name)}_{{0..{len(ens) - 1},ensemble}}/{name}.txt")


if __name__ == "__main__":
    main()
