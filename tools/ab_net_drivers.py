"""Old library against new library, one process: the host-side drivers of the network and of its training passes, bit for bit.
    python tools/ab_net_drivers.py OLD/libclasspose_hip.so classpose_amd/libclasspose_hip.so [n_subtiles[,n_subtiles...]]
Both files are PRODUCT libraries; each is loaded privately (RTLD_LOCAL), as tools/ab_libs.py loads its pair.  The weights are
built once through the package's own library (cpx_net_weights is the same struct for both).  Every buffer a driver writes
is zero-filled first and compared WHOLE, padding and staging included:
  * cpx_net_forward: workspace and head, for bf16 with the folded LayerNorm, bf16 with fuse_ln=False, fp16 and fp32, each with
    the 1x1 class head and with a [64, 128] UNet head (synthetic depth-2 checkpoints)
  * cpx_neck_forward_train (workspace = the four saved tensors, and the head) and cpx_neck_backward (gradients and workspace),
    in all three dtypes, on the backbone rows the forward left behind
  * cpx_unet_head_forward + cpx_unet_head_backward (gradients and workspace) for bf16 and fp32, on the forward's neck output
  * cpx_blocks_forward_train (workspace and head) with K = 2 and cpx_blocks_backward (gradients, dx_all and workspace) on that
    forward's record, in the four configurations of cpx_net_forward
  * at sizes of their own, whatever the list says: cpx_blocks_backward_drop, the widest backward entry, in the three precision modes (float32;
    bf16 gradients; bf16 gradients and bf16 attention backward -- the last two for the two bf16 configurations) with dx_all and dx_in at 3
    sub-tiles; cpx_blocks_forward_train_drop and cpx_blocks_backward_drop (float32 and full bf16 mode) under two masks at 5 sub-tiles and,
    bf16 folded, one at 17; cpx_embed_backward (record and workspace) in both gradient modes at 3
  * cpx_head_wgrad (dW, db and workspace) for the three feature dtypes: 3 x 1024 rows with 192 and 448 columns, 1000 rows (a short last
    slab that ends on an odd row) with 192
The default is 3 sub-tiles; 16 adds the row statistics emitted by the residual GEMMs and 33 a second MLP row part with a remainder.
One line per comparison; exit status 1 when any differs."""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from classpose_amd import _lib, engine, synth

paths = sys.argv[1:3]
SIZES = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [3]
NCLS, FTS = 7, [64, 128]
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
dev = torch.device("cuda:0")
libs = [_lib._load(os.path.abspath(p), _lib.SIGNATURES) for p in paths]
st = torch.cuda.current_stream(dev).cuda_stream
bad = 0


def zeros(n):
    return torch.zeros(int(n), dtype=torch.uint8, device=dev)


def report(what, pairs):
    """pairs: {name: (old, new)} of tensors"""
    global bad
    torch.cuda.synchronize(dev)
    same = {k: bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for k, (a, b) in pairs.items()}
    live = {k: int((b.view(torch.uint8) != 0).sum()) for k, (a, b) in pairs.items()}
    bad += not all(same.values())
    print(f"{what:44s} " + "  ".join(f"{k} {'bitwise equal' if same[k] else 'DIFFERENT'} ({b.numel() * b.element_size()} bytes, {live[k]} non-zero)"
                                    for k, (a, b) in pairs.items()), flush=True)


print(f"A = {paths[0]}\nB = {paths[1]}\ndepth-2 synthetic checkpoints, {NCLS} classes")
sds = {"1x1": synth.make_state_dict(NCLS, None, depth=2, seed=51), "unet": synth.make_state_dict(NCLS, FTS, depth=2, seed=52)}
g = torch.Generator(device=dev).manual_seed(7)
for nS in SIZES:
    print(f"--- {nS} sub-tiles")
    for prec, fuse in (("bf16", True), ("bf16", False), ("fp16", True), ("fp32", False)):
        patches = torch.randn(nS * 1024, 192, generator=g, device=dev).to(HD[prec])
        for head_kind, sd in sds.items():
            w = engine.NetWeights.from_state_dict(sd, prec, dev, fuse_ln=fuse)
            c = w.c
            tag = f"{prec}{'' if fuse or prec == 'fp32' else ' fuse_ln=False'} {head_kind}"
            out = []
            for L in libs:
                nb = L.cpx_net_workspace_bytes(nS, c.dtype) + (L.cpx_unet_workspace_bytes(c.unet_ops, c.n_unet_ops, nS, c.dtype) if c.n_unet_ops else 0)
                ws, head = zeros(nb), torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
                _lib.check(L.cpx_net_forward(C.byref(c), patches.data_ptr(), nS, head.data_ptr(), ws.data_ptr(), ws.numel(), st), "net_forward")
                out.append((ws, head))
            report(f"cpx_net_forward {tag}", {"workspace": (out[0][0], out[1][0]), "head": (out[0][1], out[1][1])})
            es = patches.element_size()
            ws = out[1][0]
            if head_kind == "1x1" and fuse == (prec != "fp32"):        # the neck's training passes, once per dtype
                o = libs[1].cpx_net_backbone_offset(nS, c.dtype)
                x = ws[o:o + nS * 1024 * 1024 * es].clone()
                dhead = torch.randn(nS * 1024, c.ld_head, generator=g, device=dev)
                n_g = libs[1].cpx_neck_grad_layout(None)
                out = []
                for L in libs:
                    fws, head = zeros(L.cpx_neck_train_workspace_bytes(nS, c.dtype)), torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_neck_forward_train(C.byref(c), x.data_ptr(), nS, head.data_ptr(), fws.data_ptr(), fws.numel(), st), "neck_forward_train")
                    bws, grads = zeros(L.cpx_neck_backward_workspace_bytes(nS, c.dtype, c.ld_head, None)), torch.zeros(n_g, dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_neck_backward(C.byref(c), x.data_ptr(), nS, fws.data_ptr(), fws.numel(), dhead.data_ptr(), grads.data_ptr(),
                                                   bws.data_ptr(), bws.numel(), st), "neck_backward")
                    out.append((fws, head, grads, bws))
                report(f"cpx_neck_forward_train {prec}", {"four tensors": (out[0][0], out[1][0]), "head": (out[0][1], out[1][1])})
                report(f"cpx_neck_backward {prec}", {"gradients": (out[0][2], out[1][2]), "workspace": (out[0][3], out[1][3])})
            if head_kind == "unet" and prec in ("bf16", "fp32") and fuse == (prec != "fp32"):
                o = libs[1].cpx_net_neck_offset(nS, c.dtype)
                feat = ws[o:o + nS * 1024 * 256 * es].clone()
                n = c.n_unet_ops
                dl = torch.randn(nS * 1024, c.unet_ops[n - 1].cout, generator=g, device=dev)
                out = []
                for L in libs:
                    fws, head = zeros(L.cpx_unet_workspace_bytes(c.unet_ops, n, nS, c.dtype)), torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_unet_head_forward(c.unet_ops, n, feat.data_ptr(), nS, head.data_ptr(), c.ld_head, 192, c.dtype, fws.data_ptr(), fws.numel(), st),
                               "unet_head_forward")
                    bws = zeros(L.cpx_unet_backward_workspace_bytes(c.unet_ops, n, nS, c.dtype))
                    grads = torch.zeros(L.cpx_unet_param_layout(c.unet_ops, n, None, None, None, None), dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_unet_head_backward(c.unet_ops, n, feat.data_ptr(), nS, c.dtype, fws.data_ptr(), fws.numel(), dl.data_ptr(), grads.data_ptr(),
                                                        bws.data_ptr(), bws.numel(), st), "unet_head_backward")
                    out.append((fws, head, grads, bws))
                report(f"cpx_unet_head_forward {prec}", {"workspace": (out[0][0], out[1][0]), "head": (out[0][1], out[1][1])})
                report(f"cpx_unet_head_backward {prec}", {"gradients": (out[0][2], out[1][2]), "workspace": (out[0][3], out[1][3])})
            if head_kind == "1x1":                                     # the blocks' training passes, in every configuration
                x = torch.randn(nS * 1024, 1024, generator=g, device=dev).to(HD[prec])
                dy0 = torch.randn(nS * 1024, 256, generator=g, device=dev)
                n_b = libs[1].cpx_block_grad_layout(None)
                params = torch.randn(2 * n_b, generator=g, device=dev) * 0.05
                out = []
                for L in libs:
                    fws, head = zeros(L.cpx_blocks_train_workspace_bytes(nS, c.dtype, 2)), torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_blocks_forward_train(C.byref(c), x.data_ptr(), nS, 0, head.data_ptr(), fws.data_ptr(), fws.numel(), st), "blocks_forward_train")
                    bws, grads = zeros(L.cpx_blocks_backward_workspace_bytes(nS, c.dtype)), torch.zeros(2 * n_b, dtype=torch.float32, device=dev)
                    dx_all = torch.zeros((3, nS * 1024, 1024), dtype=torch.float32, device=dev)
                    _lib.check(L.cpx_blocks_backward(C.byref(c), params.data_ptr(), nS, 0, fws.data_ptr(), fws.numel(), dy0.data_ptr(), grads.data_ptr(),
                                                     dx_all.data_ptr(), bws.data_ptr(), bws.numel(), st), "blocks_backward")
                    out.append((fws, head, grads, dx_all, bws))
                report(f"cpx_blocks_forward_train {tag[:-4]}", {"workspace": (out[0][0], out[1][0]), "head": (out[0][1], out[1][1])})
                report(f"cpx_blocks_backward {tag[:-4]}", {"gradients": (out[0][2], out[1][2]), "dx_all": (out[0][3], out[1][3]), "workspace": (out[0][4], out[1][4])})
                del out
            del w


def blocks_ab(tag, c, nS, prec, keep, modes):
    """The widest block-training entries on both libraries, K = 2: the forward (under ``keep``: cpx_blocks_forward_train_drop on a workspace of
    cpx_blocks_train_workspace_bytes_drop) and, per (grad_dtype, attn_grad_dtype) of ``modes``, cpx_blocks_backward_drop with dx_all and dx_in"""
    x = torch.randn(nS * 1024, 1024, generator=g, device=dev).to(HD[prec])
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=dev)
    n_b = libs[1].cpx_block_grad_layout(None)
    params = torch.randn(2 * n_b, generator=g, device=dev) * 0.05
    kp = None if keep is None else keep.ctypes.data
    fwd = []
    for L in libs:
        fws = zeros((L.cpx_blocks_train_workspace_bytes if keep is None else L.cpx_blocks_train_workspace_bytes_drop)(nS, c.dtype, 2))
        head = torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
        if keep is None:
            _lib.check(L.cpx_blocks_forward_train(C.byref(c), x.data_ptr(), nS, 0, head.data_ptr(), fws.data_ptr(), fws.numel(), st), "blocks_forward_train")
        else:
            _lib.check(L.cpx_blocks_forward_train_drop(C.byref(c), x.data_ptr(), nS, 0, kp, head.data_ptr(), fws.data_ptr(), fws.numel(), st), "blocks_forward_train_drop")
        fwd.append((fws, head))
    if keep is not None:
        report(f"cpx_blocks_forward_train_drop {tag}", {"workspace": (fwd[0][0], fwd[1][0]), "head": (fwd[0][1], fwd[1][1])})
    for gd, ad in modes:
        out = []
        for L, (fws, _) in zip(libs, fwd):
            bws, grads = zeros(L.cpx_blocks_backward_workspace_bytes_mp(nS, c.dtype, gd, ad)), torch.zeros(2 * n_b, dtype=torch.float32, device=dev)
            dx_all, dx_in = torch.zeros((3, nS * 1024, 1024), dtype=torch.float32, device=dev), torch.zeros((nS * 1024, 1024), dtype=torch.float32, device=dev)
            _lib.check(L.cpx_blocks_backward_drop(C.byref(c), params.data_ptr(), nS, 0, kp, fws.data_ptr(), fws.numel(), dy0.data_ptr(), gd, ad, grads.data_ptr(),
                                                  dx_all.data_ptr(), dx_in.data_ptr(), bws.data_ptr(), bws.numel(), st), "blocks_backward_drop")
            out.append((grads, dx_all, dx_in, bws))
        mode = "float32" if gd == _lib.DT_F32 else ("bf16 gradients" if ad == _lib.DT_F32 else "bf16 gradients + attention")
        report(f"cpx_blocks_backward_drop {tag}, {mode}", {k: (out[0][i], out[1][i]) for i, k in enumerate(("gradients", "dx_all", "dx_in", "workspace"))})


# The one-body block drivers: every precision mode through the widest entry, layer-drop masks, and the embedding's backward.  3 sub-tiles
# without a mask; 5 (slabs (0, 1), (2, 3), (4)) under a mask that gives a slab with both crops kept, the second only, the first only, none
# and the short last slab, and under one whose block 0 keeps nothing; 17, bf16 folded, with 16 and 15 crops kept: either side of the
# 16 crops from which the residual GEMMs emit the row statistics.
F32, B16 = _lib.DT_F32, _lib.DT_BF16
CONFIGS = (("bf16", True), ("bf16", False), ("fp16", True), ("fp32", False))
MASKS5 = (np.array([[1, 1, 0, 1, 1], [1, 0, 0, 0, 1]], dtype=np.uint8), np.array([[0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=np.uint8))
MASK17 = np.array([[1] * 16 + [0], [1] * 15 + [0, 0]], dtype=np.uint8)
print("--- block training: precision modes (3 sub-tiles), masks (5 and 17 sub-tiles)")
for prec, fuse in CONFIGS:
    w = engine.NetWeights.from_state_dict(sds["1x1"], prec, dev, fuse_ln=fuse)
    tag = f"{prec}{'' if fuse or prec == 'fp32' else ' fuse_ln=False'}"
    all_modes = ((F32, F32), (B16, F32), (B16, B16)) if prec == "bf16" else ((F32, F32),)
    blocks_ab(f"{tag} nS=3", w.c, 3, prec, None, all_modes)
    for i, m in enumerate(MASKS5):
        blocks_ab(f"{tag} nS=5 mask {i}", w.c, 5, prec, m, all_modes[::2])
    if (prec, fuse) == ("bf16", True):
        blocks_ab(f"{tag} nS=17 keep 16, 15", w.c, 17, prec, MASK17, all_modes[::2])
    del w
print("--- cpx_embed_backward, 3 sub-tiles")
for prec, gd in (("bf16", F32), ("bf16", B16), ("fp32", F32)):
    patches = torch.randn(3 * 1024, 192, generator=g, device=dev).to(HD[prec])
    dx_in = torch.randn(3 * 1024, 1024, generator=g, device=dev)
    out = []
    for L in libs:
        ws, grads = zeros(L.cpx_embed_backward_workspace_bytes(3, _lib.DTYPE_CODE[prec], gd)), torch.zeros(L.cpx_embed_grad_layout(None), dtype=torch.float32, device=dev)
        _lib.check(L.cpx_embed_backward(_lib.DTYPE_CODE[prec], patches.data_ptr(), dx_in.data_ptr(), 3, gd, grads.data_ptr(), ws.data_ptr(), ws.numel(), st), "embed_backward")
        out.append((grads, ws))
    report(f"cpx_embed_backward {prec}, {'float32' if gd == F32 else 'bf16'} gradients", {"record": (out[0][0], out[1][0]), "workspace": (out[0][1], out[1][1])})
print("--- cpx_head_wgrad")
for prec in ("bf16", "fp16", "fp32"):
    for rows, N in ((3 * 1024, 192), (3 * 1024, 448), (1000, 192)):
        feat = torch.randn(rows, 256, generator=g, device=dev).to(HD[prec])
        dl = torch.randn(rows, N, generator=g, device=dev)
        out = []
        for L in libs:
            ws, dW, db = zeros(L.cpx_head_wgrad_workspace_bytes(rows, N)), torch.zeros((N, 256), dtype=torch.float32, device=dev), torch.zeros(N, dtype=torch.float32, device=dev)
            _lib.check(L.cpx_head_wgrad(dl.data_ptr(), feat.data_ptr(), _lib.DTYPE_CODE[prec], rows, N, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st), "head_wgrad")
            out.append((dW, db, ws))
        report(f"cpx_head_wgrad {prec} {rows} x {N}", {"dW": (out[0][0], out[1][0]), "db": (out[0][1], out[1][1]), "workspace": (out[0][2], out[1][2])})
print("ALL BITWISE EQUAL" if not bad else f"{bad} COMPARISONS DIFFER")
sys.exit(1 if bad else 0)
