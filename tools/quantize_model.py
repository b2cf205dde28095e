#!/usr/bin/env python3
"""A QQQ W4A8 checkpoint from an fp16 one, on the GPU: a thin wrapper over qqq_amd.quant.quantize_model (GPTQ layer by layer, the
reference's examples/quant_model.py; --rotation is its rotation stage, --smooth its smoothing stage).

    python tools/quantize_model.py --config config.json --weights model.pt --tokens calib.npy --out DIR [--group-size 128]
                                   [--seqlen 2048] [--nsamples 128] [--mse] [--percdamp 0.01] [--seq-batch 1]
                                   [--rotation {none,hadamard,hadamard_k,random}] [--rotation-seed 0] [--act-order] [--static-groups]
                                   [--smooth {os+,awq,sq}] [--save-scales PATH]

--config   a transformers config.json of a Llama or Qwen2 model (read as plain JSON; transformers is not needed)
--weights  the fp16 state dict with Hugging Face parameter names: a torch.save file, or .safetensors where the safetensors package can
           be imported
--tokens   a .npy of calibration token ids of any integer dtype and shape, read in order and cut into windows of --seqlen (there is no
           tokenizer here: tokenise elsewhere)
--out      a directory: model.pt (the packed state dict, the reference's names: tools/eval_ppl.py --weights takes it) and
           quant_config.json ({"group_size", "wbits"}, as the reference writes it)
--rotation hadamard | hadamard_k | random: fuse the norms and rotate the state dict first (qqq_amd.quant.rotate_model; the reference
           runs this with --mse).  hadamard needs a power-of-two hidden size; hadamard_k takes 12, 20, 28 or 40 times a power of two as
           well (896, 1536, 3072, 3584, 5120: a Hadamard table built here mixes the K sub-blocks), and is hadamard at a power of two.  The checkpoint is then UNTIED: --out also gets config.json, the input's with "tie_word_embeddings": false, and
           quant_config.json also records {"rotation", "rotation_seed"}.  The signs / Q come from --rotation-seed.
--act-order, --static-groups   the reference's --gptq_act_order / --gptq_static_groups, which are ON by default there and off here:
           sweep the columns by falling diag(H), and find every group's scale before the sweep.  With --group-size 128, --act-order
           needs --static-groups.  The checkpoint's layout does not change; quant_config.json records the two where set.  The
           reference's default recipe is --rotation hadamard --mse --act-order --static-groups.
--smooth   os+ | awq | sq: the reference's --smooth True --smooth_method ...: search the four migration scales of every layer on the first 8
           windows (qqq_amd.quant.smooth_model), fold them into the state dict -- after --rotation where both are given -- and run GPTQ
           on the result.  The reference pairs it with its --gptq_mse False: leave --mse out.  quant_config.json records {"smooth"}.
--save-scales PATH   with --smooth: torch.save the scale_list (four fp16 vectors per layer: qkv, o, gate_up, down) there, the
           reference's scale_list.pth.
Prints one JSON line: group_size, nsamples, seqlen, linears, seconds (and rotation, smooth).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from eval_ppl import load_state_dict  # noqa: E402  (tools/eval_ppl.py: the same checkpoint formats)


def main():
    ap = argparse.ArgumentParser(description="GPTQ-quantise an fp16 Llama / Qwen2 state dict into a QQQ W4A8 checkpoint")
    ap.add_argument("--config", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--tokens", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--group-size", type=int, default=128, choices=(-1, 128))
    ap.add_argument("--seqlen", type=int, default=2048)
    ap.add_argument("--nsamples", type=int, default=128, help="at most this many windows of the token file")
    ap.add_argument("--mse", action="store_true", help="the shrink search for the scales (the reference's pairing for rotated models)")
    ap.add_argument("--percdamp", type=float, default=0.01)
    ap.add_argument("--seq-batch", type=int, default=1)
    ap.add_argument("--rotation", choices=("none", "hadamard", "hadamard_k", "random"), default="none", help="rotate the state dict before GPTQ")
    ap.add_argument("--rotation-seed", type=int, default=0)
    ap.add_argument("--act-order", action="store_true", help="sweep the columns by falling diag(H) (the reference's default; off here)")
    ap.add_argument("--static-groups", action="store_true",
                    help="find every group's scale before the sweep (the reference's default; off here; needed by --act-order with groups)")
    ap.add_argument("--smooth", choices=("os+", "awq", "sq"), default=None, help="smooth the state dict before GPTQ (after --rotation)")
    ap.add_argument("--save-scales", default=None, help="with --smooth: where to torch.save the scale_list")
    args = ap.parse_args()
    if args.save_scales and not args.smooth:
        ap.error("--save-scales needs --smooth")
    if args.act_order and args.group_size != -1 and not args.static_groups:
        ap.error("--act-order with --group-size 128 needs --static-groups (moving groups cannot be packed)")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("quantize_model.py needs a GPU: there is no CPU path")
    from qqq_amd.quant import hadamard_signs, quantize_model, random_orthogonal

    cfg = json.load(open(args.config))
    tokens = np.load(args.tokens)
    if not np.issubdtype(tokens.dtype, np.integer):
        sys.exit(f"quantize_model.py: {args.tokens} holds {tokens.dtype}, not token ids")
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
    nsamples = min(args.nsamples, tokens.size // args.seqlen)
    if nsamples < 1:
        sys.exit(f"quantize_model.py: {tokens.size} tokens are fewer than one window of {args.seqlen}")
    if tokens.min() < 0 or tokens.max() >= cfg["vocab_size"]:
        sys.exit(f"quantize_model.py: token ids outside [0, {cfg['vocab_size']})")
    ids = torch.from_numpy(tokens[:nsamples * args.seqlen].reshape(nsamples, args.seqlen))
    results = {}
    rotation = None
    if args.rotation != "none":
        gen = torch.Generator().manual_seed(args.rotation_seed)
        if args.rotation == "random":
            rotation = random_orthogonal(cfg["hidden_size"], gen)
        else:
            rotation = hadamard_signs(cfg["hidden_size"], gen)
            if args.rotation == "hadamard_k":
                rotation = ("hadamard_k", rotation)
        if not args.mse:
            print("quantize_model.py: hint: the reference pairs rotation with the scale search; consider --mse", file=sys.stderr)
    t0 = time.perf_counter()
    lm = quantize_model(load_state_dict(args.weights), SimpleNamespace(**cfg), ids, args.group_size, mse=args.mse, percdamp=args.percdamp,
                        seq_batch=args.seq_batch, results=results, rotation=rotation, act_order=args.act_order,
                        static_groups=args.static_groups, smooth=args.smooth)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.makedirs(args.out, exist_ok=True)
    torch.save({k: v.cpu() for k, v in lm.state_dict().items()}, os.path.join(args.out, "model.pt"))
    quant_config = {"group_size": args.group_size, "wbits": 4}
    summary = {"group_size": args.group_size, "nsamples": nsamples, "seqlen": args.seqlen, "linears": len(results) - (rotation is not None) - (args.smooth is not None),
               "seconds": round(dt, 2)}
    if args.act_order or args.static_groups:
        quant_config.update(act_order=args.act_order, static_groups=args.static_groups)
        summary.update(act_order=args.act_order, static_groups=args.static_groups)
    if rotation is not None:
        quant_config.update(rotation=args.rotation, rotation_seed=args.rotation_seed)
        summary.update(rotation=args.rotation)
        with open(os.path.join(args.out, "config.json"), "w") as f:  # the rotated model's lm_head is its own
            json.dump(dict(cfg, tie_word_embeddings=False), f, indent=2)
    if args.smooth:
        quant_config.update(smooth=args.smooth)
        summary.update(smooth=args.smooth)
        if args.save_scales:
            torch.save([s.cpu() for s in results["smooth"]], args.save_scales)
    with open(os.path.join(args.out, "quant_config.json"), "w") as f:
        json.dump(quant_config, f)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
