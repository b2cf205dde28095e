#!/usr/bin/env python3
"""Perplexity of a QQQ checkpoint over a file of token ids, by the protocol of the reference's examples/eval_model.py: a thin wrapper over
QuantLlamaForCausalLM.perplexity (qqq_amd/score.py).

    python tools/eval_ppl.py --config config.json --weights model.pt --tokens wikitext2_test.npy [--group-size 128] [--seqlen 2048]
                             [--kv fp16|int8] [--fuse-prefill] [--chunk-tokens 2048]
    python tools/eval_ppl.py --toy [--kv int8] [--fuse-prefill]        # a small random model and random tokens: the plumbing alone

--config   a transformers config.json of a Llama or Qwen2 model (read as plain JSON; transformers is not needed)
--weights  the checkpoint's state dict with the reference's parameter names: a torch.save file, or .safetensors where the safetensors
           package can be imported
--tokens   a .npy of token ids of any integer dtype and shape, read in order (there is no tokenizer here: tokenise elsewhere)
--group-size  -1 (per-channel) or 128; default: "group_size" of the config's "quant_config" / "quantization_config" entry
Prints one JSON line: ppl, nsamples, seqlen, kv, fuse_prefill, tokens_per_s.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOY = dict(model_type="llama", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
           num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def load_state_dict(path):
    import torch

    if path.endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError:
            sys.exit("eval_ppl.py: a .safetensors checkpoint needs the safetensors package; save the state dict with torch.save instead")
        return load_file(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def toy_model(dev):
    """a random two-layer model: random codes and scales in every QuantLinear, random embedding and head"""
    import torch

    from qqq_amd import QuantLlamaForCausalLM, pack

    lm = QuantLlamaForCausalLM.from_config(SimpleNamespace(**TOY), -1).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for mod in lm.modules():
        if hasattr(mod, "s_channel"):
            k, n = mod.infeatures, mod.outfeatures
            mod.B.copy_(pack.pack_codes(torch.randint(-7, 8, (k, n), generator=g, dtype=torch.int8, device=dev), False))
            mod.s_channel.copy_(torch.rand((1, n), generator=g, device=dev) * 4e-3 + 1e-3)
    lm.model.embed_tokens.weight.data = torch.randn((TOY["vocab_size"], TOY["hidden_size"]), generator=g, device=dev).half()
    lm.lm_head.weight.data = (0.2 * torch.randn((TOY["vocab_size"], TOY["hidden_size"]), generator=g, device=dev)).half()
    return lm.eval()


def main():
    ap = argparse.ArgumentParser(description="perplexity of a QQQ checkpoint over a .npy of token ids (the reference's eval_model.py protocol)")
    ap.add_argument("--config")
    ap.add_argument("--weights")
    ap.add_argument("--tokens")
    ap.add_argument("--group-size", type=int, default=None)
    ap.add_argument("--seqlen", type=int, default=None, help="window length (default 2048; 64 with --toy)")
    ap.add_argument("--kv", choices=("fp16", "int8"), default="fp16")
    ap.add_argument("--fuse-prefill", action="store_true")
    ap.add_argument("--chunk-tokens", type=int, default=2048)
    ap.add_argument("--toy", action="store_true", help="a random model and random tokens")
    args = ap.parse_args()
    if not args.toy and not (args.config and args.weights and args.tokens):
        ap.error("--config, --weights and --tokens are needed (or --toy)")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("eval_ppl.py needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    from qqq_amd import QuantLlamaForCausalLM

    if args.toy:
        lm = toy_model(dev)
        seqlen = args.seqlen or 64
        tokens = np.random.default_rng(0).integers(0, TOY["vocab_size"], size=8 * seqlen + 5)
    else:
        cfg = json.load(open(args.config))
        gs = args.group_size
        if gs is None:
            q = cfg.get("quant_config") or cfg.get("quantization_config") or {}
            if "group_size" not in q:
                sys.exit("eval_ppl.py: the config names no group size; pass --group-size -1 or 128")
            gs = int(q["group_size"])
        lm = QuantLlamaForCausalLM.from_config(SimpleNamespace(**cfg), gs)
        lm.load_state_dict(load_state_dict(args.weights), strict=True)
        lm = lm.to(dev).eval()
        seqlen = args.seqlen or 2048
        tokens = np.load(args.tokens)
        if not np.issubdtype(tokens.dtype, np.integer):
            sys.exit(f"eval_ppl.py: {args.tokens} holds {tokens.dtype}, not token ids")
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
    if tokens.size and (tokens.min() < 0 or tokens.max() >= lm.vocab_size):
        sys.exit(f"eval_ppl.py: token ids outside [0, {lm.vocab_size})")
    if args.fuse_prefill:
        lm.fuse_prefill()
    nsamples = tokens.size // seqlen
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppl = lm.perplexity(tokens, seqlen=seqlen, chunk_tokens=args.chunk_tokens, dtype=torch.float16 if args.kv == "fp16" else torch.int8)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"ppl": ppl, "nsamples": nsamples, "seqlen": seqlen, "kv": args.kv, "fuse_prefill": bool(args.fuse_prefill),
                      "tokens_per_s": round(nsamples * seqlen / dt, 1)}))


if __name__ == "__main__":
    main()
