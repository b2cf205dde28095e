"""Operator layer of the GPTQ quantiser over libqqq_amd_quant.so (qqq_amd/quant/include/qqq_amd_quant.h, qqq_amd_gptq_order.h,
qqq_amd_rotate.h, in qqq_amd/quant/include_ext/ qqq_amd_rotate_k.h and in qqq_amd/quant/include_ops/ qqq_amd_fakequant.h state the exact
semantics).  Every op enqueues one launch on the current stream of its tensors' device and reads nothing on the host."""
from __future__ import annotations

import torch

from ..ops import _dt, _ptr, _same_gpu, _stream_for
from . import _lib


def _raise_lib(name, err):
    if err:
        raise RuntimeError(f"qqq_amd.quant: {name} error {err}: {_lib.last_error()}")


def _matrix(name, what, t, cols=None):
    # an f32 matrix with unit column stride and a row stride that holds its columns; a view is fine, nothing is copied
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        got = f"{_dt(t.dtype)} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name}: {what} must be a float32 matrix, got {got}")
    if t.shape[0] < 1 or t.shape[1] < 1 or (cols is not None and t.shape[1] != cols):
        raise RuntimeError(f"{name}: {what} has the shape {tuple(t.shape)}" + (f", {cols} columns expected" if cols is not None else ""))
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or t.stride(0) >= 2**31:
        raise RuntimeError(f"{name}: {what} must have unit column stride and a row stride >= its columns, got strides {tuple(t.stride())}")
    if t.data_ptr() % 4:
        raise RuntimeError(f"{name}: {what} must be 4-byte aligned")
    return max(t.stride(0), t.shape[1])


def _row_vector(name, what, t, rows):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != rows or not t.is_contiguous():
        got = f"{_dt(t.dtype)} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name}: {what} must be contiguous float32 with one entry per row ({rows}), got {got}")


def weight_scales(W: torch.Tensor, grouped: bool, mse: bool = False) -> torch.Tensor:
    """The symmetric 4-bit scale of every row of `W` (f32 [rows, cols]; a column slice of a wider matrix is fine) -> f32 [rows, 1].
    grouped=False: xmax / 7 (codes -7 ... 7); grouped=True: 2 xmax / 15 (codes 0 ... 15, zero 8); xmax = max |w|, 1 for an all-zero row.
    mse=True: the reference's shrink search over 80 ranges, error |q - w| ^ 2.4, the earliest least."""
    name = "weight_scales"
    ldw = _matrix(name, "W", W)
    _same_gpu(name, (W,))
    rows, cols = W.shape
    out = torch.empty((rows, 1), dtype=torch.float32, device=W.device)
    err = _lib.lib().qqq_gptq_scales(_ptr(W), ldw, rows, cols, int(bool(grouped)), int(bool(mse)), _ptr(out), W.device.index or 0,
                                     _stream_for(W))
    _raise_lib(name, err)
    return out


def gptq_block(W1: torch.Tensor, Hinv1: torch.Tensor, scale: torch.Tensor, grouped: bool, out=None):
    """The column sweep of one GPTQ block in one launch -> (Q1, Err1), both f32 [rows, count]: new, or the pair given as `out` (views
    with their own row stride are fine: a caller may sweep into column slices of whole-matrix buffers).
    W1 f32 [rows, count] (count 64 or 128), Hinv1 f32 [count, count]: the diagonal block of the upper Cholesky factor of the inverse
    Hessian -- both may be views with their own row stride; scale f32 [rows] or [rows, 1].  Column by column: q = quantise(w, scale),
    e = (w - q) / Hinv1[i, i], the columns to the right lose e * Hinv1[i, j] (product rounded, then subtracted).  W1 is left as it is."""
    name = "gptq_block"
    ldw = _matrix(name, "W1", W1)
    rows, count = W1.shape
    if count not in (64, 128):
        raise RuntimeError(f"{name}: W1 must have 64 or 128 columns, got {count}")
    ldh = _matrix(name, "Hinv1", Hinv1, count)
    if Hinv1.shape[0] != count:
        raise RuntimeError(f"{name}: Hinv1 must be [{count}, {count}], got {tuple(Hinv1.shape)}")
    _row_vector(name, "scale", scale, rows)
    if out is None:
        out = (torch.empty((rows, count), dtype=torch.float32, device=W1.device), torch.empty((rows, count), dtype=torch.float32, device=W1.device))
    Q1, Err1 = out
    ldq, lde = _matrix(name, "Q1", Q1, count), _matrix(name, "Err1", Err1, count)
    if Q1.shape[0] != rows or Err1.shape[0] != rows:
        raise RuntimeError(f"{name}: Q1 and Err1 must have {rows} rows, got {Q1.shape[0]} and {Err1.shape[0]}")
    _same_gpu(name, (W1, Hinv1, scale, Q1, Err1))
    err = _lib.lib().qqq_gptq_block(_ptr(W1), ldw, _ptr(Hinv1), ldh, _ptr(scale), rows, count, int(bool(grouped)), _ptr(Q1), ldq,
                                    _ptr(Err1), lde, W1.device.index or 0, _stream_for(W1))
    _raise_lib(name, err)
    return Q1, Err1


def group_scales(W: torch.Tensor, mse: bool = False) -> torch.Tensor:
    """The grouped 4-bit scale (2 xmax / 15, codes 0 ... 15, zero 8) of every group of 128 columns of every row of `W` (f32 [rows, cols],
    cols a multiple of 128; a column slice of a wider matrix is fine) in one launch -> f32 [rows, cols / 128].  Entry (r, g) has the bits
    of weight_scales(W[:, 128 g : 128 g + 128], True, mse)[r]: the static groups of GPTQ, found before the sweep."""
    name = "group_scales"
    ldw = _matrix(name, "W", W)
    rows, cols = W.shape
    if cols % 128:
        raise RuntimeError(f"{name}: W has {cols} columns, no multiple of 128")
    _same_gpu(name, (W,))
    out = torch.empty((rows, cols // 128), dtype=torch.float32, device=W.device)
    err = _lib.lib().qqq_gptq_group_scales(_ptr(W), ldw, rows, cols, int(bool(mse)), _ptr(out), cols // 128, W.device.index or 0,
                                           _stream_for(W))
    _raise_lib(name, err)
    return out


def gptq_block_cols(W1: torch.Tensor, Hinv1: torch.Tensor, scales: torch.Tensor, gidx: torch.Tensor, out=None):
    """gptq_block in grouped arithmetic with a scale per (row, column): step i quantises under scales[r, gidx[i]] -> (Q1, Err1), both
    f32 [rows, count]: new, or the pair given as `out`.  W1 f32 [rows, count] (count 64 or 128), Hinv1 f32 [count, count], Q1 and Err1
    may be views with their own row strides; scales f32 [rows, groups] may be a column range of a wider table; gidx contiguous int32
    [count] on the same GPU, read on the device alone (an index outside [0, groups) is clamped into it there).  W1 is left as it is."""
    name = "gptq_block_cols"
    ldw = _matrix(name, "W1", W1)
    rows, count = W1.shape
    if count not in (64, 128):
        raise RuntimeError(f"{name}: W1 must have 64 or 128 columns, got {count}")
    ldh = _matrix(name, "Hinv1", Hinv1, count)
    if Hinv1.shape[0] != count:
        raise RuntimeError(f"{name}: Hinv1 must be [{count}, {count}], got {tuple(Hinv1.shape)}")
    lds = _matrix(name, "scales", scales)
    if scales.shape[0] != rows:
        raise RuntimeError(f"{name}: scales must have one row per row of W1 ({rows}), got {scales.shape[0]}")
    if not isinstance(gidx, torch.Tensor) or gidx.dtype != torch.int32 or gidx.dim() != 1 or gidx.numel() != count or not gidx.is_contiguous():
        got = f"{_dt(gidx.dtype)} {tuple(gidx.shape)}" if isinstance(gidx, torch.Tensor) else type(gidx).__name__
        raise RuntimeError(f"{name}: gidx must be contiguous int32 [{count}], got {got}")
    if out is None:
        out = (torch.empty((rows, count), dtype=torch.float32, device=W1.device), torch.empty((rows, count), dtype=torch.float32, device=W1.device))
    Q1, Err1 = out
    ldq, lde = _matrix(name, "Q1", Q1, count), _matrix(name, "Err1", Err1, count)
    if Q1.shape[0] != rows or Err1.shape[0] != rows:
        raise RuntimeError(f"{name}: Q1 and Err1 must have {rows} rows, got {Q1.shape[0]} and {Err1.shape[0]}")
    _same_gpu(name, (W1, Hinv1, scales, gidx, Q1, Err1))
    err = _lib.lib().qqq_gptq_block_cols(_ptr(W1), ldw, _ptr(Hinv1), ldh, _ptr(scales), lds, scales.shape[1], _ptr(gidx), rows, count,
                                         _ptr(Q1), ldq, _ptr(Err1), lde, W1.device.index or 0, _stream_for(W1))
    _raise_lib(name, err)
    return Q1, Err1


_HAD_DTYPES = {torch.float16: 0, torch.float32: 1}


def _had_matrix(name, what, t, shape=None, dtype=None):
    # an fp16 or f32 matrix with unit column stride and a row stride that holds its columns; a view is fine, nothing is copied
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in _HAD_DTYPES or (dtype is not None and t.dtype != dtype):
        got = f"{_dt(t.dtype)} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name}: {what} must be a {'float16 or float32' if dtype is None else _dt(dtype)} matrix, got {got}")
    if t.shape[0] < 1 or t.shape[1] < 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{name}: {what} has the shape {tuple(t.shape)}" + (f", {tuple(shape)} expected" if shape is not None else ""))
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or t.stride(0) >= 2**31:
        raise RuntimeError(f"{name}: {what} must have unit column stride and a row stride >= its columns, got strides {tuple(t.stride())}")
    if t.data_ptr() % t.element_size():
        raise RuntimeError(f"{name}: {what} must be aligned to its element ({t.element_size()} bytes)")
    return max(t.stride(0), t.shape[1])


def _sign_vector(name, sign, n):
    if not isinstance(sign, torch.Tensor) or sign.dtype != torch.int8 or sign.dim() != 1 or sign.numel() != n or not sign.is_contiguous():
        got = f"{_dt(sign.dtype)} {tuple(sign.shape)}" if isinstance(sign, torch.Tensor) else type(sign).__name__
        raise RuntimeError(f"{name}: sign must be contiguous int8 [{n}], got {got}")


def check_signs(sign: torch.Tensor, n: int, name: str = "check_signs") -> torch.Tensor:
    """`sign` as hadamard_rows takes it: contiguous int8 [n] with every entry +1 or -1.  The entries are READ ON THE HOST (one sync when
    the tensor is on a GPU), so this is not part of hadamard_rows: a caller checks a sign vector once, then launches as often as it likes."""
    _sign_vector(name, sign, n)
    if not bool((sign.abs() == 1).all()):
        raise RuntimeError(f"{name}: every entry of sign must be +1 or -1")
    return sign


def hadamard_rows(x: torch.Tensor, n: int, sign=None, out=None) -> torch.Tensor:
    """The Walsh-Hadamard transform of every block of `n` consecutive columns of every row of `x` (fp16 or f32 [rows, cols], cols a
    multiple of n, n a power of two 2 ... 8192; a view with its own row stride is fine) in one launch -> `out`: new, `x` itself (in
    place), or a matrix of x's shape and dtype that does not overlap it.  Per block: y = (x * sign) . H_n / sqrt(n), H the natural-order
    Sylvester matrix, summed in f64 (exactly, for fp16), divided once and rounded to f32, then to fp16: bit for bit what torch's
    `(x.double() * sign @ H / d).to(dtype)` stores wherever that product is exact.  sign: None, or int8 [n] of +-1 on x's device; its
    entries are not read here (check_signs does that, once, on the host)."""
    name = "hadamard_rows"
    ldx = _had_matrix(name, "x", x)
    rows, cols = x.shape
    if not isinstance(n, int) or n < 2 or n > 8192 or n & (n - 1):
        raise RuntimeError(f"{name}: n must be a power of two in 2 ... 8192, got {n!r}")
    if cols % n:
        raise RuntimeError(f"{name}: x has {cols} columns, no multiple of n = {n}")
    if out is None:
        out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    ldy = _had_matrix(name, "out", out, (rows, cols), x.dtype)
    if out.data_ptr() == x.data_ptr() and ldy != ldx:
        raise RuntimeError(f"{name}: out starts where x does with another row stride; in place means the same view")
    tensors = [x, out]
    if sign is not None:
        _sign_vector(name, sign, n)
        tensors.append(sign)
    _same_gpu(name, tensors)
    err = _lib.lib().qqq_hadamard_rows(_ptr(x), ldx, _ptr(out), ldy, rows, cols, n, _ptr(sign) if sign is not None else None,
                                       _HAD_DTYPES[x.dtype], x.device.index or 0, _stream_for(x))
    _raise_lib(name, err)
    return out


def _table_matrix(name, table):
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int8 or table.dim() != 2 or table.shape[0] != table.shape[1] or not table.is_contiguous():
        got = f"{_dt(table.dtype)} {tuple(table.shape)}" if isinstance(table, torch.Tensor) else type(table).__name__
        raise RuntimeError(f"{name}: table must be contiguous int8 [K, K], got {got}")
    K = table.shape[0]
    if K % 4 or K < 4 or K > 64:
        raise RuntimeError(f"{name}: table has K = {K}, no multiple of 4 in 4 ... 64")
    return K


def check_table(table: torch.Tensor, name: str = "check_table") -> torch.Tensor:
    """`table` as hadamard_rows_k takes it: contiguous int8 [K, K], K a multiple of 4 in 4 ... 64, every entry +1 or -1, and Hadamard:
    table . table^T == K I in integer arithmetic.  The entries are READ ON THE HOST (one sync when the tensor is on a GPU), so this is
    not part of hadamard_rows_k: a caller checks a table once, then launches as often as it likes."""
    K = _table_matrix(name, table)
    if not bool((table.abs() == 1).all()):
        raise RuntimeError(f"{name}: every entry of table must be +1 or -1")
    t = table.cpu().to(torch.int64)
    if not torch.equal(t @ t.t(), K * torch.eye(K, dtype=torch.int64)):
        raise RuntimeError(f"{name}: table is no Hadamard matrix (table . table^T != {K} I)")
    return table


def hadamard_rows_k(x: torch.Tensor, m: int, table: torch.Tensor, sign=None, out=None) -> torch.Tensor:
    """hadamard_rows for blocks of n = K * m columns, K no power of two: every block of `x` (fp16 or f32 [rows, cols], cols a multiple
    of n <= 8192; a view with its own row stride is fine) becomes (x * sign) . (table^T (x) H_m) / sqrt(n) in one launch -> `out`: new,
    `x` itself (in place), or a matrix of x's shape and dtype that does not overlap it.  H_m is the natural-order Sylvester matrix on
    every sub-block of m = 2^p >= 1 entries; `table` (int8 [K, K] of +-1 on x's device, K a multiple of 4 in 4 ... 64) then mixes the
    K sub-blocks: y[k m + c] = sum_k' table[k][k'] t[k' m + c], k' ascending, in f64 (exactly, for fp16), divided once and rounded to
    f32, then to fp16 -- the reference's matmul_hadU with hadK = table.  sign: None, or int8 [n] of +-1.  Neither the table's nor the
    signs' entries are read here (check_table and check_signs do that, once, on the host)."""
    name = "hadamard_rows_k"
    ldx = _had_matrix(name, "x", x)
    rows, cols = x.shape
    K = _table_matrix(name, table)
    if not isinstance(m, int) or m < 1 or m & (m - 1) or K * m > 8192:
        raise RuntimeError(f"{name}: m must be a power of two with K * m = {K} * m <= 8192, got {m!r}")
    n = K * m
    if cols % n:
        raise RuntimeError(f"{name}: x has {cols} columns, no multiple of n = {n}")
    if out is None:
        out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    ldy = _had_matrix(name, "out", out, (rows, cols), x.dtype)
    if out.data_ptr() == x.data_ptr() and ldy != ldx:
        raise RuntimeError(f"{name}: out starts where x does with another row stride; in place means the same view")
    tensors = [x, out, table]
    if sign is not None:
        _sign_vector(name, sign, n)
        tensors.append(sign)
    _same_gpu(name, tensors)
    err = _lib.lib().qqq_hadamard_rows_k(_ptr(x), ldx, _ptr(out), ldy, rows, cols, K, m, _ptr(table), _ptr(sign) if sign is not None else None,
                                         _HAD_DTYPES[x.dtype], x.device.index or 0, _stream_for(x))
    _raise_lib(name, err)
    return out


def _fq_matrix(name, what, t, shape=None):
    # an fp16 matrix of 16-byte units: unit column stride, a row stride that holds its columns and is a multiple of 8, a 16-byte aligned base
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float16:
        got = f"{_dt(t.dtype)} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name}: {what} must be a float16 matrix, got {got}")
    if t.shape[0] < 1 or t.shape[1] < 8 or t.shape[1] % 8 or t.shape[1] > 2**30 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{name}: {what} has the shape {tuple(t.shape)}" + (f", {tuple(shape)} expected" if shape is not None else
                                                                                 ", the columns must be a multiple of 8 in 8 ... 2^30"))
    ld = max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or ld % 8 or ld >= 2**31:
        raise RuntimeError(f"{name}: {what} must have unit column stride and a row stride >= its columns that is a multiple of 8, got strides {tuple(t.stride())}")
    if t.data_ptr() % 16:
        raise RuntimeError(f"{name}: {what} must be 16-byte aligned")
    return ld


def fake_quant_rows(x: torch.Tensor, col_scale, bits: int, group: int = 0, divide: bool = False, out=None) -> torch.Tensor:
    """The reference's MigratorBase.quantize of a column-scaled operand in one launch: `x` (fp16 [rows, cols], cols a multiple of 8; a view
    with its own row stride, a multiple of 8, is fine) divided (divide=True, the activation side) or multiplied (the weight side) by
    `col_scale` (None, or contiguous fp16 [cols] on x's device), then fake-quantised symmetrically to `bits` (8 or 4: codes -127 ... 127 or
    -7 ... 7) with one scale per row (group=0) or per (row, 128 columns) (group=128, cols a multiple of 128) -> `out`: new, `x` itself (in
    place), or a matrix of x's shape that does not overlap it.  Every step is one f32 operation rounded to fp16, as torch evaluates the
    reference's fp16 expression (qqq_amd_fakequant.h states each): the result has the bits of the torch composition, and holds no -0."""
    name = "fake_quant_rows"
    ldx = _fq_matrix(name, "x", x)
    rows, cols = x.shape
    if bits not in (4, 8):
        raise RuntimeError(f"{name}: bits must be 8 or 4, got {bits!r}")
    if group not in (0, 128):
        raise RuntimeError(f"{name}: group must be 0 (one scale per row) or 128, got {group!r}")
    if group and cols % group:
        raise RuntimeError(f"{name}: x has {cols} columns, no multiple of group = {group}")
    if out is None:
        out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    ldy = _fq_matrix(name, "out", out, (rows, cols))
    if out.data_ptr() == x.data_ptr() and ldy != ldx:
        raise RuntimeError(f"{name}: out starts where x does with another row stride; in place means the same view")
    tensors = [x, out]
    if col_scale is not None:
        if (not isinstance(col_scale, torch.Tensor) or col_scale.dtype != torch.float16 or col_scale.dim() != 1 or col_scale.numel() != cols
                or not col_scale.is_contiguous()):
            got = f"{_dt(col_scale.dtype)} {tuple(col_scale.shape)}" if isinstance(col_scale, torch.Tensor) else type(col_scale).__name__
            raise RuntimeError(f"{name}: col_scale must be None or contiguous float16 [{cols}], got {got}")
        if col_scale.data_ptr() % 16:
            raise RuntimeError(f"{name}: col_scale must be 16-byte aligned")
        tensors.append(col_scale)
    _same_gpu(name, tensors)
    err = _lib.lib().qqq_fake_quant_rows(_ptr(x), ldx, _ptr(out), ldy, rows, cols, _ptr(col_scale) if col_scale is not None else None,
                                         bits, group, int(bool(divide)), x.device.index or 0, _stream_for(x))
    _raise_lib(name, err)
    return out
