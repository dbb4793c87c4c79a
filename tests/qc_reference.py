"""TEST INFRASTRUCTURE ONLY -- float64 interpreter of ``cpx_qc_op`` programs (csrc/cpx_qc.hip) and the synthetic
single-op programs the host and GPU tests share.

The interpreter restates what ``cpx_qc_forward`` documents, op by op, on a host copy of the workspace (a flat numpy
array of floats; float32 when it mirrors the device, float64 when a whole program is interpreted without rounding the
activations).  Every op returns its result in float64 together with a per-element error bound for a float32 device:

u = 2^-24, K = products per output element, S = the same operation on absolute values (sum |a g w| + |bias|).

* dense / depthwise pre-activation: (K + 3) u S + 1e-30 -- the order-independent bound of a float32 dot product
  ((K - 1) u S for the additions in any order, u S for the products unless fused), + the gate multiply, the bias add
  and the final rounding, one u S each.
* ReLU: monotone and 1-Lipschitz, adds nothing.
* SiLU v / (1 + e), e = __expf(-v) = hardware exp2 of fl(log2e * v): the argument carries the rounding of the product
  and of the constant (<= 1.2 u |v| log2e, i.e. <= 1.5 u |v| relative in e), the instruction 1 ulp (<= 2 u), so e is
  within (1.5 |v| + 2) u; 1 + e and the division round once each and e / (1 + e) <= 1, so the value is within
  (1.5 |v| + 4) u <= (2 |v| + 8) u relative; the pre-activation error passes through the slope (<= 1.0999):
  1.1 e_pre + (2 |v| + 8) u |silu(v)| + 1e-30 (the 1e-30 also covers results flushed to -0 below v = -87).
* sigmoid 1 / (1 + e): slope <= 1/4, same relative term: e_s / 4 + (2 |s| + 8) u sigmoid(s) + 1e-30.
* residual: one more rounding, u (|res| + |value|).
* squeeze-excite: the same constants step by step: mean ((HW + 2) u mean|x|; with integer inputs whose sums stay below
  2^24 every partial sum is exact in any order and only 1 / HW and the product round: (2 u + u^2) |mean|), reduce
  (|w1| e_mean + (C + 3) u (|w1| |mean| + |b1|)), SiLU, expand (|w2| e_red + (Cr + 3) u (|w2| |red| + |b2|)), sigmoid.

``defect=`` makes the interpreter wrong on purpose in one plausible way; the host tests use it to show that the inputs
of every synthetic case would expose such a kernel (tests/test_qc_program_host.py::test_detection_power_*)."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from classpose_amd._lib import CpxQcOp
from classpose_amd.grandqc import NONE, _pad16, pack_dense_weights, pack_dw_weights

U = 2.0 ** -24
TINY = 1e-30
SENT = -7777.25
MEAN = np.array((0.485, 0.456, 0.406))
STD = np.array((0.229, 0.224, 0.225))
KIND = {0: "dense", 1: "depthwise", 2: "squeeze-excite"}


class Region(NamedTuple):
    """channel slice [0, c) of ``rows`` rows of ``ld`` floats starting at float index ``off`` of the workspace"""
    off: int
    rows: int
    ld: int
    c: int

    def end(self) -> int:
        return self.off + (self.rows - 1) * self.ld + self.c

    def view(self, ws: np.ndarray) -> np.ndarray:
        assert self.off >= 0 and self.end() <= ws.size, (self, ws.size)
        return np.lib.stride_tricks.as_strided(ws[self.off:], shape=(self.rows, self.c),
                                               strides=(self.ld * ws.itemsize, ws.itemsize))

    def mark(self, mask: np.ndarray, value=True) -> None:
        self.view(mask)[...] = value


def _floats(byte_off: int) -> int:
    assert byte_off % 4 == 0, byte_off
    return byte_off // 4


def op_regions(op, nB: int) -> dict:
    """what one op reads ('a', 'b', 'gate', 'res') and writes ('dst', for kind 2 also 'pool')"""
    P = nB * op.h_out * op.w_out
    r = {}
    if op.kind == 0:
        sh = 1 if op.up_a else 0
        r["a"] = Region(_floats(op.src_a), nB * (op.h_in >> sh) * (op.w_in >> sh), op.ld_a, op.c_a)
        if op.src_b != NONE:
            r["b"] = Region(_floats(op.src_b), nB * op.h_in * op.w_in, op.ld_b, op.c_b)
        if op.gate != NONE:
            r["gate"] = Region(_floats(op.gate), nB, op.c_a, op.c_a)
        if op.res != NONE:
            r["res"] = Region(_floats(op.res), P, op.ld_res, op.c_out)
        r["dst"] = Region(_floats(op.dst), P, op.ld_dst, op.c_out)
    elif op.kind == 1:
        r["a"] = Region(_floats(op.src_a), nB * op.h_in * op.w_in, op.ld_a, op.c_a)
        r["dst"] = Region(_floats(op.dst), P, op.c_a, op.c_a)
    elif op.kind == 2:
        r["a"] = Region(_floats(op.src_a), nB * op.h_in * op.w_in, op.ld_a, op.c_a)
        r["pool"] = Region(_floats(op.res), 16 * nB, op.c_a, op.c_a)
        r["dst"] = Region(_floats(op.dst), nB, op.c_a, op.c_a)
    else:
        raise ValueError(f"unknown kind {op.kind}")
    return r


def written(op, nB: int) -> list:
    r = op_regions(op, nB)
    return [r["dst"]] + ([r["pool"]] if "pool" in r else [])


# ---- the operations -------------------------------------------------------------------------------
def pre(patches_u8: np.ndarray) -> np.ndarray:
    """k_qc_pre: ((u8 / 255) - mean) / std in float64, cast to float32, zero fourth channel; (n, H, W, 4)"""
    x = (patches_u8.astype(np.float64) / 255.0 - MEAN) / STD
    out = np.zeros(patches_u8.shape[:3] + (4,), np.float32)
    out[..., :3] = x.astype(np.float32)
    return out


def act_apply(v: np.ndarray, e: np.ndarray, act: int):
    if act == 0:
        return v, e
    if act == 1:
        return np.maximum(v, 0.0), e
    assert act == 2, act
    with np.errstate(over="ignore"):
        sv = v / (1.0 + np.exp(-v))
    return sv, 1.1 * e + (2.0 * np.abs(v) + 8.0) * U * np.abs(sv) + TINY


def sigmoid_apply(s: np.ndarray, e: np.ndarray):
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-s))
    return g, 0.25 * e + (2.0 * np.abs(s) + 8.0) * U * g + TINY


def _taps(x: np.ndarray, k: int, stride: int, pad: int, h_out: int, w_out: int, inside_tap=None):
    """x (n, h, w, c) -> for every tap the (n, h_out, w_out, c) gather, zero outside the image.  ``inside_tap`` =
    (tap, oy, ox): that one tap of that one output pixel reads the nearest pixel inside the image instead (a defect)."""
    n, h, w, c = x.shape
    for ky in range(k):
        iy = np.arange(h_out) * stride - pad + ky
        vy = (iy >= 0) & (iy < h)
        for kx in range(k):
            ix = np.arange(w_out) * stride - pad + kx
            vx = (ix >= 0) & (ix < w)
            m = vy[:, None] & vx[None, :]
            if inside_tap is not None and inside_tap[0] == ky * k + kx:
                m = m.copy()
                assert not m[inside_tap[1], inside_tap[2]], "the defect's tap must be a border tap"
                m[inside_tap[1], inside_tap[2]] = True
            g = x[:, np.clip(iy, 0, h - 1)][:, :, np.clip(ix, 0, w - 1)]
            yield ky * k + kx, np.where(m[None, :, :, None], g, 0.0)


def dense(ws: np.ndarray, op, nB: int, wts, defect: str | None = None) -> dict:
    r = op_regions(op, nB)
    sh = 1 if op.up_a else 0
    a = r["a"].view(ws).astype(np.float64).reshape(nB, op.h_in >> sh, op.w_in >> sh, op.c_a)
    if op.up_a:
        a = a.repeat(2, axis=1).repeat(2, axis=2)
    if "gate" in r:
        g = r["gate"].view(ws).astype(np.float64)
        if defect == "gate_image0":
            g = g.copy()
            g[-1] = g[0]
        a = a * g[:, None, None, :]
    if defect == "tail12_zero":
        assert op.c_a % 16 == 12
        a = a.copy()
        a[..., op.c_a - 4:] = 0.0
    c_b = op.c_b if "b" in r else 0
    x = a
    if c_b:
        x = np.concatenate([a, r["b"].view(ws).astype(np.float64).reshape(nB, op.h_in, op.w_in, c_b)], axis=-1)
    taps = op.k * op.k
    apad, bpad = _pad16(op.c_a), (_pad16(c_b) if c_b else 0)
    tn = 32 if op.c_out <= 32 else 64
    cpad = (op.c_out + tn - 1) // tn * tn
    wp = np.asarray(wts(op.w), np.float64).reshape(cpad, taps, apad + bpad)
    b0 = apad - 4 if defect == "b_offset" else apad
    w = np.concatenate([wp[:op.c_out, :, :op.c_a], wp[:op.c_out, :, b0:b0 + c_b]], axis=-1)     # [cout][tap][cin]
    bias = np.asarray(wts(op.bias), np.float64)[:op.c_out] if op.bias else np.zeros(op.c_out)
    P = nB * op.h_out * op.w_out
    acc = np.broadcast_to(bias, (P, op.c_out)).copy()
    S = np.abs(acc)
    for t, xt in _taps(x, op.k, op.stride, op.pad, op.h_out, op.w_out):
        xt = xt.reshape(P, -1)
        acc += xt @ w[:, t, :].T
        S += np.abs(xt) @ np.abs(w[:, t, :]).T
    K = taps * (op.c_a + c_b)
    e_pre = (K + 3) * U * S + TINY
    val, e = act_apply(acc, e_pre, op.act)
    if "res" in r:
        res = r["res"].view(ws).astype(np.float64)
        e = e + U * (np.abs(res) + np.abs(val))
        val = val + res
    return dict(ref=val, tol=e, pre=acc, S=S, K=K)


def depthwise(ws: np.ndarray, op, nB: int, wts, defect: str | None = None) -> dict:
    r = op_regions(op, nB)
    C_ = op.c_a
    x = r["a"].view(ws).astype(np.float64).reshape(nB, op.h_in, op.w_in, C_)
    taps = op.k * op.k
    w = np.asarray(wts(op.w), np.float64).reshape(taps, C_)
    bias = np.asarray(wts(op.bias), np.float64)[:C_]
    acc = np.broadcast_to(bias, (nB, op.h_out, op.w_out, C_)).copy()
    S = np.abs(acc)
    inside = (0, 0, 0) if defect == "border_tap" else None       # top-left tap of the top-left output pixel
    for t, xt in _taps(x, op.k, op.stride, op.pad, op.h_out, op.w_out, inside):
        acc += xt * w[t]
        S += np.abs(xt) * np.abs(w[t])
    P = nB * op.h_out * op.w_out
    acc, S = acc.reshape(P, C_), S.reshape(P, C_)
    e_pre = (taps + 3) * U * S + TINY
    val, e = act_apply(acc, e_pre, op.act)
    return dict(ref=val, tol=e, pre=acc, S=S, K=taps)


def pool_slices(hw: int) -> int:
    return 16 if hw >= 16384 else (4 if hw >= 1024 else 1)


def squeeze_excite(ws: np.ndarray, op, nB: int, wts, defect: str | None = None) -> dict:
    r = op_regions(op, nB)
    C_, Cr, HW = op.c_a, op.c_red, op.h_in * op.w_in
    x = r["a"].view(ws).astype(np.float64).reshape(nB, HW, C_)
    slices = pool_slices(HW)
    per = (HW + slices - 1) // slices
    part = np.zeros((16, nB, C_))
    for z in range(slices):
        p0, p1 = z * per, min(HW, (z + 1) * per)
        if defect == "pool_last_pixel" and z == slices - 1:
            p1 -= 1
        part[z] = x[:, p0:p1].sum(1)
    exact = bool(np.all(x == np.rint(x))) and float(np.abs(x).sum(1).max()) < 2.0 ** 24
    mean = part.sum(0) / HW
    e_mean = ((2 * U + U * U) * np.abs(mean) if exact else (HW + 2) * U * np.abs(x).mean(1)) + TINY
    w1 = np.asarray(wts(op.w), np.float64).reshape(Cr, C_)
    b1 = np.asarray(wts(op.bias), np.float64)[:Cr]
    w2 = np.asarray(wts(op.w2), np.float64).reshape(C_, Cr)
    b2 = np.asarray(wts(op.bias2), np.float64)[:C_]
    v = mean @ w1.T + b1
    e_v = e_mean @ np.abs(w1).T + (C_ + 3) * U * (np.abs(mean) @ np.abs(w1).T + np.abs(b1)) + TINY
    red, e_red = act_apply(v, e_v, 2)
    s = red @ w2.T + b2
    e_s = e_red @ np.abs(w2).T + (Cr + 3) * U * (np.abs(red) @ np.abs(w2).T + np.abs(b2)) + TINY
    g, e_g = sigmoid_apply(s, e_s)
    return dict(ref=g, tol=e_g, pool=part.reshape(16 * nB, C_), pool_rows=slices * nB, exact=exact, mean=mean, s=s)


def run_op(ws: np.ndarray, op, nB: int, wts, defect: str | None = None) -> dict:
    return (dense, depthwise, squeeze_excite)[op.kind](ws, op, nB, wts, defect)


def argmax(ws: np.ndarray, logits_off: int, npix: int, ld: int, n_classes: int) -> np.ndarray:
    """first maximum wins over the first n_classes of ld lanes"""
    return np.argmax(Region(_floats(logits_off), npix, ld, n_classes).view(ws), axis=1).astype(np.int8)


def interpret(ops, nB: int, patches_u8: np.ndarray, input_off: int, ws_floats: int, wts, dtype=np.float64) -> np.ndarray:
    """the whole program on a fresh NaN workspace of ``dtype`` (float64: activations are never rounded)"""
    ws = np.full(ws_floats, np.nan, dtype)
    H, W = patches_u8.shape[1:3]
    Region(_floats(input_off), nB * H * W, 4, 4).view(ws)[...] = pre(patches_u8).reshape(-1, 4)
    for op in ops:
        out = run_op(ws, op, nB, wts)
        op_regions(op, nB)["dst"].view(ws)[...] = out["ref"]
    return ws


# ---- weights behind raw pointers -------------------------------------------------------------------
class Weights:
    """keeps float32 tensors on a device and resolves their raw pointers again (what QcNet._keep /
    QcNet.weight_tensor do for a planned network)"""

    def __init__(self, device):
        self.device = torch.device(device)
        self.keep: dict = {}
        self._host: dict = {}

    def put(self, t) -> int:
        t = torch.as_tensor(t).to(torch.float32).contiguous().to(self.device)
        self.keep[t.data_ptr()] = t
        return t.data_ptr()

    def __call__(self, p: int) -> np.ndarray:
        if p not in self._host:
            self._host[p] = self.keep[p].cpu().numpy()
        return self._host[p]


def net_weights(net):
    cache: dict = {}

    def get(p: int) -> np.ndarray:
        if p not in cache:
            cache[p] = net.weight_tensor(p).cpu().numpy()
        return cache[p]
    return get


# ---- synthetic single-op programs --------------------------------------------------------------------
class Case:
    """a workspace image + ops + the mandatory pre / argmax geometry (H = W = 32)"""

    def __init__(self, device, nB: int, seed: int, n_classes: int = 2):
        self.nB, self.H, self.W = nB, 32, 32
        self.n_classes, self.ld_logits = n_classes, (n_classes + 3) // 4 * 4
        self.rng = np.random.default_rng(seed)
        self.wts = Weights(device)
        self.ops: list = []
        self.labels: list = []
        self._chunks: list = []
        self._cursor = 0
        self.patches = self.rng.integers(0, 256, (nB, 32, 32, 3), dtype=np.uint8)
        self.input = self.tensor(nB * 1024, 4, 4, fill=SENT)
        self.logits = self.tensor(nB * 1024, self.ld_logits, self.ld_logits, fill=0.0)

    def tensor(self, rows: int, ld: int, c: int, off: int = 0, data=None, fill=np.nan) -> Region:
        """a buffer of rows x ld floats (``fill`` everywhere, ``data`` in the channel slice [off, off + c)), followed
        by a guard of 64 sentinel floats"""
        assert off + c <= ld and off % 4 == 0
        buf = np.full((rows, ld), fill, np.float32)
        if data is not None:
            buf[:, off:off + c] = np.asarray(data, np.float32).reshape(rows, c)
        n = (rows * ld + 63) // 64 * 64 + 64
        flat = np.full(n, SENT, np.float32)
        flat[:rows * ld] = buf.ravel()
        reg = Region(self._cursor + off, rows, ld, c)
        self._chunks.append(flat)
        self._cursor += n
        return reg

    def add(self, label: str, **kw) -> None:
        base = dict(k=1, stride=1, pad=0, act=0, src_b=NONE, gate=NONE, res=NONE, up_a=0, c_b=0, ld_b=0, ld_res=0,
                    c_red=0, w2=None, bias2=None)
        base.update(kw)
        self.ops.append(CpxQcOp(**base))
        self.labels.append(label)

    def finish(self) -> "Case":
        self.ws = np.concatenate(self._chunks)
        self.ws_bytes = self.ws.size * 4
        self.input_off, self.logits_off = self.input.off * 4, self.logits.off * 4
        return self


def _out(n: int, stride: int) -> int:
    return (n + stride - 1) // stride


def add_dense(cs: Case, h_in: int, w_in: int, c_a: int, c_out: int, k: int = 1, stride: int = 1, act: int = 0,
              pad_a: int = 8, up: int = 0, c_b: int = 0, gate: bool = False, res: bool = False, pad_dst: int = 8,
              label: str = "") -> None:
    """one dense op on fresh buffers: A is the slice [4, 4 + c_a) of rows of c_a + pad_a floats (NaN around it), B the
    slice that ends its rows of c_b + 40 floats, the residual a slice of rows of c_out + 12 floats, the destination the
    slice [4, 4 + c_out) of rows of c_out + pad_dst sentinels.  SiLU gets biases spread over [-12, 12]."""
    rng, nB = cs.rng, cs.nB
    sh = 1 if up else 0
    ha, wa = h_in >> sh, w_in >> sh
    h_out, w_out = _out(h_in, stride), _out(w_in, stride)
    P = nB * h_out * w_out
    off_a = 4 if pad_a else 0
    A = cs.tensor(nB * ha * wa, c_a + pad_a, c_a, off_a, rng.standard_normal((nB * ha * wa, c_a)))
    kw = {}
    if c_b:
        B = cs.tensor(nB * h_in * w_in, c_b + 40, c_b, 40, rng.standard_normal((nB * h_in * w_in, c_b)))
        kw.update(src_b=B.off * 4, c_b=c_b, ld_b=B.ld)
    if gate:
        G = cs.tensor(nB, c_a, c_a, 0, rng.uniform(0.05, 0.95, (nB, c_a)))
        kw.update(gate=G.off * 4)
    if res:
        R = cs.tensor(P, c_out + 12, c_out, 4, rng.standard_normal((P, c_out)))
        kw.update(res=R.off * 4, ld_res=R.ld)
    D = cs.tensor(P, c_out + pad_dst, c_out, 4 if pad_dst else 0, fill=SENT)
    cin = c_a + c_b
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    w = torch.randn((c_out, cin, k, k), generator=g, dtype=torch.float64) / math.sqrt(cin * k * k)
    scale = 1.0 + 0.1 * torch.randn(c_out, generator=g, dtype=torch.float64)
    shift = 0.3 * torch.randn(c_out, generator=g, dtype=torch.float64)
    if act == 2:
        shift = shift + torch.linspace(-12.0, 12.0, c_out, dtype=torch.float64)
    wp, bp = pack_dense_weights(w, scale, shift, c_a, c_b, label)
    cs.add(label or f"dense c_a={c_a} c_out={c_out}", kind=0, k=k, stride=stride, pad=k // 2, act=act, h_in=h_in,
           w_in=w_in, h_out=h_out, w_out=w_out, src_a=A.off * 4, dst=D.off * 4, c_a=c_a, ld_a=A.ld, up_a=up,
           c_out=c_out, ld_dst=D.ld, w=cs.wts.put(wp), bias=cs.wts.put(bp), **kw)


def add_depthwise(cs: Case, h: int, w: int, C_: int, k: int, stride: int, pad_a: int = 8, label: str = "") -> None:
    rng, nB = cs.rng, cs.nB
    h_out, w_out = _out(h, stride), _out(w, stride)
    A = cs.tensor(nB * h * w, C_ + pad_a, C_, 4 if pad_a else 0, rng.standard_normal((nB * h * w, C_)))
    D = cs.tensor(nB * h_out * w_out, C_, C_, 0, fill=SENT)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    wt = torch.randn((C_, 1, k, k), generator=g, dtype=torch.float64) / k
    scale = 1.0 + 0.1 * torch.randn(C_, generator=g, dtype=torch.float64)
    shift = 3.0 * torch.randn(C_, generator=g, dtype=torch.float64)
    wp, bp = pack_dw_weights(wt, scale, shift)
    cs.add(label or f"depthwise {h}x{w} C={C_} k={k} s={stride} ld_a={A.ld}", kind=1, k=k, stride=stride, pad=k // 2,
           act=2, h_in=h, w_in=w, h_out=h_out, w_out=w_out, src_a=A.off * 4, dst=D.off * 4, c_a=C_, ld_a=A.ld,
           c_out=C_, ld_dst=C_, w=cs.wts.put(wp), bias=cs.wts.put(bp))


def add_se(cs: Case, h: int, w: int, C_: int, c_red: int, integer: bool = True, pad_a: int = 8, label: str = "") -> None:
    rng, nB = cs.rng, cs.nB
    HW = h * w
    if integer:
        x = rng.integers(-8, 9, (nB * HW, C_)).astype(np.float64)
        x.reshape(nB, HW, C_)[:, -1] = np.where(rng.random((nB, C_)) < 0.5, -8.0, 8.0)   # the last pixel counts
    else:
        x = rng.standard_normal((nB * HW, C_)) + 0.5
        x.reshape(nB, HW, C_)[:, -1] = np.where(rng.random((nB, C_)) < 0.5, -1.0, 1.0) * rng.uniform(6.0, 8.0, (nB, C_))
    A = cs.tensor(nB * HW, C_ + pad_a, C_, 4 if pad_a else 0, x)
    pool = cs.tensor(16 * nB, C_, C_, 0, fill=SENT)
    G = cs.tensor(nB, C_, C_, 0, fill=SENT)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    f = 24.0 if integer else 2.0                                  # integer means are O(8 / sqrt(HW)): scale them up
    w1 = f * torch.randn((c_red, C_), generator=g, dtype=torch.float64) / math.sqrt(C_)
    b1 = torch.randn(c_red, generator=g, dtype=torch.float64)
    w2 = torch.randn((C_, c_red), generator=g, dtype=torch.float64) / math.sqrt(c_red)
    b2 = torch.randn(C_, generator=g, dtype=torch.float64)
    cs.add(label or f"squeeze-excite HW={HW} C={C_} c_red={c_red}", kind=2, h_in=h, w_in=w, h_out=1, w_out=1,
           src_a=A.off * 4, res=pool.off * 4, dst=G.off * 4, c_a=C_, ld_a=A.ld, c_out=C_, ld_dst=C_, c_red=c_red,
           w=cs.wts.put(w1), bias=cs.wts.put(b1), w2=cs.wts.put(w2), bias2=cs.wts.put(b2))


# the synthetic programs, by name; the GPU tests run them on the device, the host tests show their detection power
TILE_P = {35: (1, 5, 7), 105: (3, 5, 7), 128: (2, 8, 8), 351: (3, 9, 13)}
TILE_COUT = (2, 8, 24, 32, 40, 64, 80, 112)
SRC_CA = (4, 12, 16, 24, 28, 40, 136)
SE_EXACT = {35: (5, 7, 96, 4), 1023: (33, 31, 144, 6), 1024: (32, 32, 1152, 48), 1085: (35, 31, 16, 1),
            16384: (128, 128, 16, 4), 16512: (129, 128, 16, 1)}


def case_dense_tiles(device, P: int) -> Case:
    nB, h, w = TILE_P[P]
    cs = Case(device, nB, 100 + P)
    for c_out in TILE_COUT:
        add_dense(cs, h, w, 24, c_out, label=f"dense tiles P={P} c_out={c_out}")
    return cs.finish()


def case_dense_sources(device, k: int, stride: int) -> Case:
    cs = Case(device, 2, 200 + 10 * k + stride)
    for c_a in SRC_CA:
        for (h, w) in ((2, 3), (9, 13)):
            if c_a == 136 and (h, w) == (2, 3):
                continue
            add_dense(cs, h, w, c_a, 24, k=k, stride=stride, label=f"dense sources c_a={c_a} {h}x{w} k={k} s={stride}")
    return cs.finish()


def case_dense_upsample(device) -> Case:
    cs = Case(device, 2, 300)
    for c_a, c_b in ((40, 0), (28, 24), (16, 48), (12, 24)):
        add_dense(cs, 6, 4, c_a, 40, k=3, act=1, up=1, c_b=c_b, label=f"dense up_a c_a={c_a} c_b={c_b}")
    return cs.finish()


def case_dense_gate_residual(device) -> Case:
    cs = Case(device, 3, 400)
    for c_a, c_out in ((144, 24), (28, 80), (12, 16)):
        add_dense(cs, 5, 7, c_a, c_out, gate=True, res=True, label=f"dense gate+residual c_a={c_a} c_out={c_out}")
    return cs.finish()


def case_dense_acts(device) -> Case:
    cs = Case(device, 2, 500)
    for act in (0, 1, 2):
        add_dense(cs, 9, 13, 24, 96, k=3, act=act, label=f"dense act={act}")
    return cs.finish()


def case_depthwise(device, k: int, stride: int) -> Case:
    cs = Case(device, 3, 600 + 10 * k + stride)
    for C_ in (4, 32, 144):
        for (h, w) in ((2, 3), (1, 1), (9, 13)):
            for pad_a in (0, 8):
                add_depthwise(cs, h, w, C_, k, stride, pad_a)
    return cs.finish()


def case_se_exact(device, HW: int) -> Case:
    h, w, C_, cr = SE_EXACT[HW]
    cs = Case(device, 3, 700 + HW % 97)
    add_se(cs, h, w, C_, cr)
    return cs.finish()


def case_se_real(device) -> Case:
    cs = Case(device, 3, 800)
    add_se(cs, 35, 31, 96, 4, integer=False)
    return cs.finish()
