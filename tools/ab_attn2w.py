"""One-process interleaved A/B of the production attention kernel (variant 2, k_attention2w: two query rows per wave, two
workgroups per CU) against the round-2/3 kernel (variant 7, k_attention4p): the attention launch alone (V^T already in place,
as in the engine) and the whole engine step (tools/ab_engine.py), both orders in alternate rounds.

    python tools/ab_attn2w.py [rounds=9] [n_subtiles=32] [A=2] [B=7]"""
import os as _os
_os.environ.setdefault("CLASSPOSE_HIP_DEBUG", "1")      # variant 7 lives in the -DCPX_DEBUG library
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from classpose_amd import _lib, engine, ops, synth

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
nS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
dev = torch.device("cuda:0")
L = _lib.lib()
A = int(sys.argv[3]) if len(sys.argv) > 3 else 2
B = int(sys.argv[4]) if len(sys.argv) > 4 else 7
st = torch.cuda.current_stream().cuda_stream

# ---- attention alone: cpx_attention = the V transpose kernel (identical for both variants, ~10 us) + the attention kernel
g = torch.Generator().manual_seed(3)
qkv = (torch.randn(nS * 1024, 3072, generator=g) * 0.7).to(torch.bfloat16).to(dev)
rel = (torch.randn(64, 64, generator=g) * 0.8).to(torch.bfloat16).to(dev); rel[63] = 0
vt = torch.empty((nS * 1024, 1024), dtype=torch.bfloat16, device=dev); out = torch.empty_like(vt)
outs = {}
for v in (A, B):
    L.cpx_attention_set_variant(v)
    outs[v] = ops.attention(qkv, rel, rel)
print(f"outputs bitwise equal: {bool(torch.equal(outs[A], outs[B]))}")


def time_attention(v, n=20):
    L.cpx_attention_set_variant(v)
    for _ in range(3):
        L.cpx_attention(0, qkv.data_ptr(), rel.data_ptr(), rel.data_ptr(), nS, vt.data_ptr(), out.data_ptr(), st)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * n)]
    for i in range(n):
        ev[2 * i].record()
        L.cpx_attention(0, qkv.data_ptr(), rel.data_ptr(), rel.data_ptr(), nS, vt.data_ptr(), out.data_ptr(), st)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(n)]))


t_att = {A: [], B: []}
for rnd in range(rounds):
    for v in ((A, B) if rnd % 2 == 0 else (B, A)):
        t_att[v].append(time_attention(v))
L.cpx_attention_set_variant(2)
for v in (A, B):
    print(f"attention variant {v}: median {np.median(t_att[v]):7.1f} us  min {min(t_att[v]):7.1f}  (V transpose + attention, {nS} sub-tiles)  "
          f"all {[round(x, 1) for x in t_att[v]]}")

# ---- the whole engine step (configs[1] shape: 8 tiles of 256^2 -> 32 sub-tiles, depth 24)
sd = synth.make_state_dict(7, None, depth=24, seed=0)
w = engine.NetWeights.from_state_dict(sd, "bf16", dev)
eng = engine.Engine(w, 256, batch_tiles=8)
tiles = torch.from_numpy(np.stack([synth.render_region(1234, 224 * i, 0, 256, 256) for i in range(8)])).to(dev)


def run(n):
    prev = None
    for i in range(n):
        sid = eng.submit(tiles)
        if prev is not None: eng.result(prev)
        prev = sid
    eng.result(prev)
    torch.cuda.synchronize()


res = {A: [], B: []}
for rnd in range(rounds):
    for v in ((A, B) if rnd % 2 == 0 else (B, A)):
        L.cpx_attention_set_variant(v)
        run(2)
        t = time.perf_counter(); run(10); dt = (time.perf_counter() - t) / 10
        res[v].append(dt * 1e3)
L.cpx_attention_set_variant(2)
for v in (A, B):
    print(f"engine step variant {v}: ms/step median {np.median(res[v]):.3f} min {min(res[v]):.3f}  all {[round(x, 2) for x in res[v]]}")
for o, name in ((0, "A first"), (1, "B first")):
    d = [res[B][i] - res[A][i] for i in range(o, rounds, 2)]
    print(f"engine step, rounds with {name}: variant {B} - variant {A} = median {np.median(d):.3f} ms  min {min(d):.3f}")
