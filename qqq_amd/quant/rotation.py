"""Rotation in front of GPTQ: the reference's QQQ/rotation/rotation.py over plain state dicts (Hugging Face parameter names, the way
quant/model.py works without transformers).  fuse_layer_norms folds every RMSNorm weight into the linears behind it, rotate_state_dict
turns the residual stream by an orthogonal Q (embeddings, lm_head, q/k/v, gate/up: W <- W Q;  o_proj, down_proj: W <- Q^T W) and then
applies the per-head Hadamard to v_proj (output side) and o_proj (input side).  The function the model computes does not change, the
norms are all ones and every weight keeps its shape: the result loads into the same modules and needs no kernel at inference.

With Q = diag(s) H / d (mode="hadamard", the reference's default; s random signs, H the Sylvester matrix, d = sqrt(hidden)) every
product with Q is one launch of ops.hadamard_rows instead of the reference's O(n^2) f64 matmul, and the per-head step is the same op
with n = head_dim in place of the reference's CUDA package.  Every other Q (mode="random", an explicit matrix) takes the reference's
line in torch, `(W.double() @ Q).to(dtype)`, and still the op for the per-head step.

Where the bits differ from the reference's:
  * its per-head step is an f32 butterfly inside a CUDA package (fast_hadamard_transform) whose rounding order is its own; ours is the
    exact sum divided once and rounded once, so single fp16 elements can differ by one ulp.  That cannot be measured here (no CUDA);
    against an f32 product with the Sylvester matrix as a stand-in, tests/golden/rotate_small.npz records how many do.
  * for a hidden size that is an odd power of two (d is not a power of two) its f64 matmul rounds every product w * (1 / d) and then
    the sums, while we divide the exact sum once.  The fp16 results agree on the fixture (32 x 128, bit for bit).
A power-of-four hidden size (64, 1024, 4096) gives the reference's Q-stage bits exactly: both are exact sums scaled by a power of two.

Hidden sizes K * 2^p (mode="hadamard_k": 896, 1536, 3072, 3584, 5120 ...).  The reference multiplies by hadK (x) H_m there, hadK one of
its literal K x K tables.  ops.hadamard_rows_k takes the table as an argument and does the sub-block stages and the K-mix in one
launch; hadamard_table builds OUR tables for K = 12, 20, 28, 40 by construction (Paley I, Paley II, Sylvester doubling).
  * OUR TABLES DIFFER FROM THE REFERENCE'S (no plain Paley construction gives its tables, their transposes or negatives): Q is another
    matrix, equally orthogonal.  A checkpoint carries no Q -- the rotation is folded into the weights -- so nothing downstream depends
    on which table was used.  Given the reference's table (`table=`), the Q stage has the reference's bits wherever its per-product
    rounding agrees with one divide of the exact sum (tests/golden/rotate_k_small.npz records the count of elements where not).

Not here: tables of other orders than 12, 20, 28, 40 (a caller may pass any Hadamard matrix of order K <= 64), a head_dim that is no
power of two, any online Hadamard.  (Smoothing is the next stage: smooth.py, applied to the rotated state dict.)"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

_RIGHT = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight")
_LEFT = ("self_attn.o_proj", "mlp.down_proj")  # weight and bias
_HEAD_NORMS = ("self_attn.q_norm.weight", "self_attn.k_norm.weight")  # Qwen3: carried through, folded nowhere
_FUSED_BY = {"input_layernorm.weight": ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"),
             "post_attention_layernorm.weight": ("mlp.gate_proj.weight", "mlp.up_proj.weight")}


def _is_pow2(n: int) -> bool:
    return n > 0 and n & (n - 1) == 0


def _check_dtype(name, key, t):
    if t.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{name}: {key} is {str(t.dtype).replace('torch.', '')}; only float16 and float32 state dicts are rotated")


def _layer_prefixes(state_dict) -> list:
    idx = sorted({int(k.split(".")[2]) for k in state_dict if k.startswith("model.layers.")})
    return [f"model.layers.{i}." for i in idx]


def fuse_layer_norms(state_dict: dict, config) -> dict:
    """A new state dict with every RMSNorm weight folded into the linears that read the norm's output, `(W.double() * g.double())
    .to(dtype)` as the reference: input_layernorm into q/k/v, post_attention_layernorm into gate/up, model.norm into lm_head; the norm
    weights become ones.  Tensors that do not change are shared with the input, nothing is modified in place.

    THE RESULT IS UNTIED.  With `config.tie_word_embeddings`, or without an lm_head.weight in the input, the result gets an
    lm_head.weight of its own: a copy of the embedding made before anything is fused, which then takes model.norm.  The embedding stays
    as it was (the reference, given a tied matrix, folds the norm into the embedding as well and later rotates it twice).  Build the
    model that loads the result with tie_word_embeddings = False."""
    name = "fuse_layer_norms"
    out = dict(state_dict)
    if bool(getattr(config, "tie_word_embeddings", False)) or "lm_head.weight" not in state_dict:
        out["lm_head.weight"] = state_dict["model.embed_tokens.weight"].clone()

    def fuse(norm_key, linear_keys):
        g = out[norm_key]
        _check_dtype(name, norm_key, g)
        for k in linear_keys:
            W = out[k]
            _check_dtype(name, k, W)
            out[k] = (W.double() * g.to(W.device).double()).to(W.dtype)
        out[norm_key] = torch.ones_like(g)

    for prefix in _layer_prefixes(state_dict):
        for norm, linears in _FUSED_BY.items():
            fuse(prefix + norm, [prefix + k for k in linears])
    fuse("model.norm.weight", ["lm_head.weight"])
    return out


def hadamard_signs(n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int8 [n] of +-1, uniform: the diagonal of the reference's random_hadamard_matrix (on the CPU; seed the generator to repeat it)"""
    return (torch.randint(0, 2, (n,), generator=generator) * 2 - 1).to(torch.int8)


def random_orthogonal(n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """f64 [n, n]: the Q of a QR decomposition of a normal matrix with the signs of diag(R) folded in (the reference's mode "random")"""
    q, r = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, generator=generator))
    return q * torch.sign(torch.diag(r)).unsqueeze(0)


def hadamard_matrix(signs: torch.Tensor) -> torch.Tensor:
    """f64 [n, n]: diag(signs) H / d, the matrix the Hadamard path multiplies by without forming it (for checks and for the dense path
    of another tool); d = sqrt(n) in f32, as the op"""
    n = signs.numel()
    i = torch.arange(n)
    bits = i[:, None] & i[None, :]
    par = torch.zeros_like(bits)
    while bool(bits.any()):
        par ^= bits & 1
        bits = bits >> 1
    H = (1 - 2 * par).double()
    return signs.double()[:, None] * H / torch.tensor(n).sqrt().double()


_TABLE_ORDERS = (28, 40, 20, 12)  # the reference's precedence among the tables built here
_NOT_BUILT = (172, 156, 140, 108, 60, 52, 36)  # the reference's other tables, which it tries first


def _jacobsthal(q: int) -> torch.Tensor:
    # [q, q] of chi(i - j): the quadratic character of the prime field GF(q), 0 on the diagonal
    squares = {x * x % q for x in range(1, q)}
    chi = [0] + [1 if a in squares else -1 for a in range(1, q)]
    return torch.tensor([[chi[(i - j) % q] for j in range(q)] for i in range(q)], dtype=torch.int64)


def _paley(q: int) -> torch.Tensor:
    """Paley I for a prime q = 3 (mod 4): I + S of order q + 1, S = [[0, 1], [-1, J]] skew; Paley II for a prime q = 1 (mod 4):
    S = [[0, 1], [1, J]] symmetric, every entry replaced by a 2 x 2 block, of order 2 (q + 1); J the Jacobsthal matrix"""
    S = torch.zeros((q + 1, q + 1), dtype=torch.int64)
    S[0, 1:] = 1
    S[1:, 0] = -1 if q % 4 == 3 else 1
    S[1:, 1:] = _jacobsthal(q)
    eye = torch.eye(q + 1, dtype=torch.int64)
    if q % 4 == 3:
        return S + eye
    return torch.kron(S, torch.tensor([[1, 1], [1, -1]])) + torch.kron(eye, torch.tensor([[1, -1], [-1, -1]]))


def hadamard_table(K: int) -> torch.Tensor:
    """int8 [K, K] of +-1, a Hadamard matrix of order K in {12, 20, 28, 40}, built by construction: Paley I over GF(11) and GF(19),
    Paley II over GF(13), and the Sylvester double of the order-20 one.  NOT the reference's literal tables (see the module's text)."""
    if K == 12:
        H = _paley(11)
    elif K == 20:
        H = _paley(19)
    elif K == 28:
        H = _paley(13)
    elif K == 40:
        H = torch.kron(torch.tensor([[1, 1], [1, -1]]), _paley(19))
    else:
        raise RuntimeError(f"hadamard_table: no table of order K = {K!r} is built here (12, 20, 28 and 40 are); pass your own as table=")
    return ops.check_table(H.to(torch.int8).contiguous(), "hadamard_table")


def hadamard_factor(n: int):
    """(K, m) with n = K * m, m a power of two: the table order the reference's get_hadK picks for n among those built here (28, then
    40, then 20, then 12), or K = 1 for a power of two.  An n the reference sends to a table that is not built here (a multiple of
    172, 156, 140, 108, 60, 52 or 36, which it tries first) and an n that is none of these raise by name."""
    name = "hadamard_factor"
    if not isinstance(n, int) or n < 1:
        raise RuntimeError(f"{name}: n must be a positive integer, got {n!r}")
    for K in _NOT_BUILT:
        if n % K == 0:
            raise RuntimeError(f"{name}: n = {n} is a multiple of {K}: the reference takes its table of order {K} there, and none of that "
                               "order is built here; pass a Hadamard matrix of an order K <= 64 that divides n as table=")
    for K in _TABLE_ORDERS:
        if n % K == 0:
            if not _is_pow2(n // K):
                raise RuntimeError(f"{name}: n = {n} = {K} * {n // K}, and {n // K} is not a power of two; pass a Hadamard matrix of an "
                                   "order K <= 64 with n / K a power of two as table=")
            return K, n // K
    if not _is_pow2(n):
        raise RuntimeError(f"{name}: n = {n} is neither a power of two nor 12, 20, 28 or 40 times one; pass a Hadamard matrix of an "
                           "order K <= 64 with n / K a power of two as table=")
    return 1, n


def hadamard_matrix_k(signs: torch.Tensor, table: torch.Tensor, m: int) -> torch.Tensor:
    """f64 [n, n], n = K m: diag(signs) (table^T (x) H_m) / d, the matrix mode="hadamard_k" multiplies by without forming it (for
    checks and for the dense path of another tool); d = sqrt(n) in f32, as the op.  With the reference's table it is the reference's
    random_hadamard_matrix for these signs."""
    K = table.shape[0]
    n = K * m
    if signs.numel() != n:
        raise RuntimeError(f"hadamard_matrix_k: {signs.numel()} signs for n = {K} * {m} = {n}")
    H = (hadamard_matrix(torch.ones(m, dtype=torch.int8)) * torch.tensor(m).sqrt().double()).round()  # the +-1 Sylvester matrix
    M = torch.kron(table.cpu().double().t().contiguous(), H)
    return signs.cpu().double()[:, None] * M / torch.tensor(n).sqrt().double()


def _had(W, n, sign, dev, table=None):
    # the op on a 2-D tensor from anywhere: computed on `dev`, returned where W lives, W itself untouched
    if table is not None:
        return ops.hadamard_rows_k(W.to(dev).contiguous(), n // table.shape[0], table, sign=sign).to(W.device)
    return ops.hadamard_rows(W.to(dev).contiguous(), n, sign=sign).to(W.device)


def rotate_state_dict(state_dict: dict, config, mode: str = "hadamard", signs: Optional[torch.Tensor] = None,
                      Q: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, device=None,
                      table: Optional[torch.Tensor] = None):
    """The rotated copy of an UNTIED state dict whose norm weights are ones (fuse_layer_norms makes one) -> (dict, signs or Q).

    mode="hadamard": Q = diag(signs) H / sqrt(hidden); `signs` int8 [hidden] of +-1, or drawn from `generator` (hadamard_signs); the
    hidden size must be a power of two up to 8192.  Returns the signs.  mode="random": Q from random_orthogonal(hidden, generator).  An
    explicit `Q` (f64 [hidden, hidden], orthogonal: not checked) overrides the mode.  Both return Q, and take the reference's dense line.
    mode="hadamard_k": hidden = K * 2^p up to 8192; Q = diag(signs) (table^T (x) H_m) / sqrt(hidden), one launch of
    ops.hadamard_rows_k per weight.  `table` int8 [K, K], a Hadamard matrix (checked: ops.check_table) whose order divides hidden into a
    power of two; None: hadamard_factor(hidden) picks K and hadamard_table(K) builds it.  For a power-of-two hidden size without a table
    the mode IS "hadamard".  Returns the signs.
    Then the per-head Hadamard of size head_dim on v_proj (output side, weight and bias) and o_proj (input side), each a separate
    rounding to the weight's dtype, as the reference rounds between the two steps.

    float16 and float32 tensors; every tensor is computed on `device` (default cuda:0: the op has no CPU path) and returned where it
    lived.  Tensors that do not change are shared with the input."""
    name = "rotate_state_dict"
    dev = torch.device(device if device is not None else "cuda:0")
    hidden = config.hidden_size
    heads = config.num_attention_heads
    head_dim = getattr(config, "head_dim", None) or hidden // heads
    if not _is_pow2(head_dim) or head_dim < 2:
        raise RuntimeError(f"{name}: head_dim = {head_dim} is not a power of two: the per-head Hadamard needs one")
    if "lm_head.weight" not in state_dict:
        raise RuntimeError(f"{name}: the state dict has no lm_head.weight; a tied model is untied by fuse_layer_norms first")
    if mode not in ("hadamard", "hadamard_k", "random"):
        raise RuntimeError(f"{name}: mode must be 'hadamard', 'hadamard_k' or 'random', got {mode!r}")
    dense = Q is not None or mode == "random"
    if signs is not None and dense:
        raise RuntimeError(f"{name}: signs belong to mode='hadamard' without an explicit Q")
    if table is not None and (dense or mode != "hadamard_k"):
        raise RuntimeError(f"{name}: table belongs to mode='hadamard_k' without an explicit Q")
    table_dev = None
    if dense:
        if Q is None:
            Q = random_orthogonal(hidden, generator)
        if not isinstance(Q, torch.Tensor) or Q.dtype != torch.float64 or tuple(Q.shape) != (hidden, hidden):
            raise RuntimeError(f"{name}: Q must be a float64 [{hidden}, {hidden}] matrix")
        Qd = Q.to(dev)
        sign_dev = None
    else:
        if mode == "hadamard_k":
            if not isinstance(hidden, int) or hidden < 1 or hidden > 8192:
                raise RuntimeError(f"{name}: hidden_size = {hidden} is not in 1 ... 8192")
            if table is not None:
                ops.check_table(table, name)  # the one host read of the table
                K = table.shape[0]
                if hidden % K or not _is_pow2(hidden // K):
                    raise RuntimeError(f"{name}: hidden_size = {hidden} is not the table's order {K} times a power of two")
            else:
                try:
                    K, _ = hadamard_factor(hidden)
                except RuntimeError as e:
                    raise RuntimeError(f"{name}: hidden_size: {e}") from None
                if K > 1:
                    table = hadamard_table(K)
        elif not _is_pow2(hidden) or hidden > 8192:
            raise RuntimeError(f"{name}: hidden_size = {hidden} is not a power of two up to 8192; the Paley-type Hadamard tables the "
                               "reference uses for sizes K * 2^p are not part of the repository: mode='hadamard_k' builds its own for "
                               "K = 12, 20, 28, 40 or takes one as table=; for any other size use mode='random'")
        if signs is None:
            signs = hadamard_signs(hidden, generator)
        ops.check_signs(signs, hidden, name)  # the one host read of the signs
        sign_dev = signs.to(dev)
        table_dev = table.to(dev) if table is not None else None

    def right(W):  # W Q
        if dense:
            return (W.to(dev).double() @ Qd).to(W.dtype).to(W.device)
        return _had(W, hidden, sign_dev, dev, table_dev)

    def left(W):  # Q^T W, a bias as a column
        if dense:
            return (Qd.T @ W.to(dev).double()).to(W.dtype).to(W.device)
        if W.dim() == 1:
            return _had(W.unsqueeze(0), hidden, sign_dev, dev, table_dev).squeeze(0)
        return _had(W.t(), hidden, sign_dev, dev, table_dev).t().contiguous()

    out = dict(state_dict)
    for k, W in state_dict.items():
        tail = k.split(".", 3)[3] if k.startswith("model.layers.") and k.count(".") >= 4 else None
        if k in ("model.embed_tokens.weight", "lm_head.weight") or tail in _RIGHT:
            _check_dtype(name, k, W)
            out[k] = right(W)
        elif tail is not None and tail.rsplit(".", 1)[0] in _LEFT:
            _check_dtype(name, k, W)
            out[k] = left(W)
        elif tail in _HEAD_NORMS:
            pass  # Qwen3's q_norm / k_norm act per head on a projection's OUTPUT: the residual rotation is on the input side, the per-head
            # Hadamard on v / o only, so they pass through as they are (and need not be ones)
        elif k.endswith("norm.weight") or k.endswith("layernorm.weight"):
            if not bool((W == 1).all()):
                raise RuntimeError(f"{name}: {k} is not all ones: a rotation commutes with RMSNorm only after fuse_layer_norms")
    # the reference's rotate_ov_proj: H_head on the output side of v_proj and the input side of o_proj, each block of head_dim
    for prefix in _layer_prefixes(state_dict):
        v, o = prefix + "self_attn.v_proj.", prefix + "self_attn.o_proj."
        out[v + "weight"] = _had(out[v + "weight"].t(), head_dim, None, dev).t().contiguous()
        if v + "bias" in out:
            _check_dtype(name, v + "bias", out[v + "bias"])
            out[v + "bias"] = _had(out[v + "bias"].unsqueeze(0), head_dim, None, dev).squeeze(0)
        out[o + "weight"] = _had(out[o + "weight"], head_dim, None, dev)
    return out, (Q if dense else signs)


def rotate_model(state_dict: dict, config, mode: str = "hadamard", signs: Optional[torch.Tensor] = None, Q: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None, device=None, table: Optional[torch.Tensor] = None):
    """fuse_layer_norms, then rotate_state_dict -> (dict, signs or Q).  The result is UNTIED (see fuse_layer_norms)."""
    return rotate_state_dict(fuse_layer_norms(state_dict, config), config, mode=mode, signs=signs, Q=Q, generator=generator, device=device,
                             table=table)
