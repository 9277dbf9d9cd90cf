#!/usr/bin/env python3
"""Drop-in for the reference's _downstream_tasks/SS/predict.py (RNA-MSM-SS) on MI355X.

    python SS_predict.py --rootdir DIR --featdir results --rnaid 2DRB_1 --device cuda [--gemm-dtype bf16]
                         [--nested [--nested-threshold X] [--nested-min-loop N]]

Reads `<featdir>/<rnaid>.fasta` (each record's description is its name) and `<featdir>/<rnaid>_atp.npy` (the [120, L, L]
maps RNA_MSM_Inference.py writes), runs the 16-block head of `<rootdir>/model/rna-msm_attention.pt` on the HIP device
(rnamsm.ss.SSPredictor) and writes `<featdir>/SS_result/<name>.{ct,bpseq,prob}` as the reference does.
--nested: also the nested (pseudoknot-free) structure of greatest summed pair probability above the threshold, decoded on the device
(rnamsm.ss.nested_structure): `SS_result/<name>.dbn` (dot-bracket), `<name>.nested.ct` and `<name>.nested.bpseq`.
Not supported: `--plots` (the reference's VARNA drawings need a Java jar) and any device but the HIP one.
"""
import os
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "rna-msm_amd"))


def get_args(argv=None):
    p = ArgumentParser()
    p.add_argument("--rootdir", default=ROOT, type=str, help="weights at <rootdir>/model/rna-msm_attention.pt")
    p.add_argument("--featdir", default=os.path.join(ROOT, "results"), type=str)
    p.add_argument("--rnaid", default="2DRB_1", type=str)
    p.add_argument("--plots", default="False", type=str, help="not supported here (VARNA plots)")
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the HIP device; there is no CPU path)")
    p.add_argument("--gemm-dtype", default="f32", type=str,
                   help="arithmetic of the head's convolutions: f32 (exact, default) or bf16 (bf16 matrix cores, fp32 accumulation)")
    p.add_argument("--nested", action="store_true", help="also write <name>.dbn, <name>.nested.ct and <name>.nested.bpseq")
    p.add_argument("--nested-threshold", default=0.516, type=float, help="pairs count by their probability above this, in [0, 1)")
    p.add_argument("--nested-min-loop", default=3, type=int, help="fewest unpaired bases a hairpin encloses, in [0, 32]")
    return p.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    if args.plots.strip().lower() not in ("false", "0", "no", ""):
        sys.exit("SS_predict.py: --plots is not supported (the VARNA drawings need the reference's Java tool); "
                 "the .ct file it would draw is written as usual")
    if not args.device.startswith("cuda"):
        sys.exit(f"SS_predict.py: --device {args.device}: this build runs on the HIP device only (--device cuda)")
    from rnamsm.config import SS_GEMM_DTYPES
    if args.gemm_dtype not in SS_GEMM_DTYPES:
        sys.exit(f"SS_predict.py: --gemm-dtype {args.gemm_dtype}: not one of {', '.join(SS_GEMM_DTYPES)}")
    from rnamsm.config import check_ss_nested
    try:
        check_ss_nested(args.nested, args.nested_threshold, args.nested_min_loop, "given")
    except ValueError as e:
        sys.exit("SS_predict.py: " + str(e).replace("data.ss_nested_threshold", "--nested-threshold").replace("data.ss_nested_min_loop", "--nested-min-loop"))
    import numpy as np
    import torch
    from rnamsm import ss
    from rnamsm.msa import read_fasta_records

    fasta = os.path.join(args.featdir, args.rnaid + ".fasta")
    atp_path = os.path.join(args.featdir, args.rnaid + "_atp.npy")
    model_path = os.path.join(args.rootdir, "model", "rna-msm_attention.pt")
    for path in (fasta, atp_path, model_path):
        if not os.path.isfile(path):
            sys.exit(f"SS_predict.py: {path} not found")
    device = torch.device(args.device)
    model = ss.load_predictor(model_path, device, gemm_dtype=args.gemm_dtype)
    print(f"SS head arithmetic: {args.gemm_dtype}")
    atp = np.load(atp_path)
    if atp.ndim != 3 or atp.shape[0] != ss.NUM_MAPS or atp.shape[1] != atp.shape[2]:
        sys.exit(f"SS_predict.py: {atp_path} holds an array of shape {atp.shape}, not [{ss.NUM_MAPS}, L, L]")
    atp_dev = torch.from_numpy(np.ascontiguousarray(atp, dtype=np.float32)).to(device)
    for name, seq in read_fasta_records(fasta):
        if len(seq) != atp.shape[-1]:
            sys.exit(f"SS_predict.py: {name}: sequence of length {len(seq)} but attention maps of L = {atp.shape[-1]} "
                     f"in {atp_path}")
        with torch.no_grad():
            prob, partner, counts, ct_body, bpseq_body = (t.cpu().numpy() for t in model.predict_structure(atp_dev, seq))
        ss.write_ss_files(prob, seq, name, args.featdir, partner=partner, counts=counts, ct_body=ct_body, bpseq_body=bpseq_body)
        print(f"{name}: {os.path.join(args.featdir, 'SS_result', name)}.{{ct,bpseq,prob}}")
        if args.nested:
            probs_dev = torch.from_numpy(prob).to(device)
            letters = torch.from_numpy(ss.letter_codes(seq)).to(device)
            nested = ss.nested_structure(probs_dev, letters, args.nested_threshold, args.nested_min_loop)
            ss.write_nested_files(seq, name, args.featdir, *(t.cpu().numpy() for t in nested))
            print(f"{name}: {os.path.join(args.featdir, 'SS_result', name)}.{{dbn,nested.ct,nested.bpseq}}")


if __name__ == "__main__":
    main()
