"""The workspace layouts of the network drivers and of the training passes, pinned to literal values.  Host only: every
query here is plain arithmetic inside the library, so the library answers without a device.

The forward drivers, the neck's and the UNet head's training passes and the post-processing / metrics / dedup / label
statistics entries each lay their workspace out through a few shared pieces (cpx_net_ws, op_dims, CpxArena).  Callers
allocate by these numbers and read saved activations at these offsets, so the numbers are part of the ABI: a change to
the shared pieces must not move them.

EXPECTED was recorded from the library of the commit before the layouts were shared (the block-training and head weight-gradient
entries: of the commit before the block launch sequence was shared), by this file itself:
    python tests/test_layout_host.py path/to/libclasspose_hip.so
prints the table for any product library (the op list comes from the package on disk; the answers from the library named).
"""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from classpose_amd import _lib, engine, synth  # noqa: E402

DTYPES = {"bf16": 0, "fp16": 1, "fp32": 2}
SIZE_MAX = 2 ** 64 - 1                      # (size_t)-1
LD_HEAD = 640


def unet_ops():
    """the op list of a fts = [64, 128], 7-class UNet head, built on the CPU as tests/test_host_logic.py builds its lists"""
    w = engine.NetWeights.from_state_dict(synth.make_state_dict(7, [64, 128], depth=1, seed=4), "fp32", "cpu")
    return w, w.unet_ops, w.c.n_unet_ops


def layout_table(L):
    """{query: answer} for the library L"""
    t = {}
    sz4 = C.c_size_t * 4
    for name, dt in DTYPES.items():
        for nS in (1, 3, 32):
            fwd, bwd = sz4(), sz4()
            assert L.cpx_neck_train_layout(nS, dt, fwd) == 0
            bwd_bytes = L.cpx_neck_backward_workspace_bytes(nS, dt, LD_HEAD, bwd)
            t[f"net {name} {nS}"] = (L.cpx_net_workspace_bytes(nS, dt), L.cpx_net_neck_offset(nS, dt), L.cpx_net_backbone_offset(nS, dt),
                                     L.cpx_neck_train_workspace_bytes(nS, dt), tuple(fwd), bwd_bytes, tuple(bwd))
    keep, ops, n = unet_ops()
    ll, ii = C.c_longlong * n, C.c_int * n
    w_off, b_off, n_pad, k_pad = ll(), ll(), ii(), ii()
    t["unet params"] = (L.cpx_unet_param_layout(ops, n, w_off, b_off, n_pad, k_pad), tuple(w_off), tuple(b_off), tuple(n_pad), tuple(k_pad))
    for name, dt in DTYPES.items():
        for nS in (1, 3):
            g_off, g_ld = (C.c_size_t * n)(), ii()
            assert L.cpx_unet_grad_layout(ops, n, nS, dt, g_off, g_ld) == 0
            t[f"unet {name} {nS}"] = (L.cpx_unet_workspace_bytes(ops, n, nS, dt), L.cpx_unet_backward_workspace_bytes(ops, n, nS, dt),
                                      tuple(g_off), tuple(g_ld))
    del keep
    t["postproc (3, 224, 224)"] = L.cpx_postproc_workspace_bytes(3, 224, 224)
    t["pq (2, 256, 256, 6, 4096)"] = L.cpx_pq_workspace_bytes(2, 256, 256, 6, 4096)
    t["dedup (1000, 37, 41)"] = L.cpx_dedup_pairs_workspace_bytes(1000, 37, 41)
    t["label_stats (2, 256, 256, 6)"] = L.cpx_label_stats_workspace_bytes(2, 256, 256, 6)
    # block training: the forward's record of K trained blocks, the backward's slab workspace and the pieces it is made of
    for name, dt in DTYPES.items():
        for nS in (1, 3, 32):
            for K in (1, 2):
                off = (C.c_size_t * (4 * K + 2))()
                assert L.cpx_blocks_train_layout(nS, dt, K, off) == 0
                t[f"blocks {name} {nS} K={K}"] = (L.cpx_blocks_train_workspace_bytes(nS, dt, K), tuple(off))
        t[f"blocks backward {name}"] = (L.cpx_blocks_backward_workspace_bytes(1, dt), L.cpx_blocks_backward_workspace_bytes(32, dt))
    g_off = (C.c_longlong * 14)()
    t["blocks pieces"] = (L.cpx_blocks_backward_slab_crops(), L.cpx_block_grad_layout(g_off), tuple(g_off),
                          L.cpx_attention_backward_workspace_bytes(2), L.cpx_layernorm_backward_bytes(2048, 1024))
    t["head_wgrad (1000, 448) (8192, 192) (1000, 100)"] = (L.cpx_head_wgrad_workspace_bytes(1000, 448), L.cpx_head_wgrad_workspace_bytes(8192, 192),
                                                          L.cpx_head_wgrad_workspace_bytes(1000, 100))
    # invalid arguments: 0, and (size_t)-1 where 0 is a valid offset
    t["invalid"] = (L.cpx_net_workspace_bytes(0, 0), L.cpx_net_neck_offset(0, 0), L.cpx_net_neck_offset(1, 3), L.cpx_net_neck_offset(1, -1),
                    L.cpx_net_backbone_offset(0, 2), L.cpx_net_backbone_offset(1, 3), L.cpx_net_backbone_offset(1, -1),
                    L.cpx_neck_train_workspace_bytes(0, 0), L.cpx_neck_train_workspace_bytes(1, 3),
                    L.cpx_neck_backward_workspace_bytes(1, 0, 100, None), L.cpx_neck_backward_workspace_bytes(1, 3, LD_HEAD, None),
                    L.cpx_unet_workspace_bytes(None, 0, 1, 0), L.cpx_unet_backward_workspace_bytes(None, 0, 1, 0))
    return t


EXPECTED = {'blocks backward bf16': (253112320, 253112320),
 'blocks backward fp16': (253112320, 253112320),
 'blocks backward fp32': (253112320, 253112320),
 'blocks bf16 1 K=1': (29392896, (0, 2097152, 8388608, 10485760, 12582912, 14680064)),
 'blocks bf16 1 K=2': (41975808, (0, 2097152, 8388608, 10485760, 12582912, 14680064, 20971520, 23068672, 25165824, 27262976)),
 'blocks bf16 3 K=1': (88178688, (0, 6291456, 25165824, 31457280, 37748736, 44040192)),
 'blocks bf16 3 K=2': (125927424, (0, 6291456, 25165824, 31457280, 37748736, 44040192, 62914560, 69206016, 75497472, 81788928)),
 'blocks bf16 32 K=1': (940572672, (0, 67108864, 268435456, 335544320, 402653184, 469762048)),
 'blocks bf16 32 K=2': (1343225856, (0, 67108864, 268435456, 335544320, 402653184, 469762048, 671088640, 738197504, 805306368, 872415232)),
 'blocks fp16 1 K=1': (29392896, (0, 2097152, 8388608, 10485760, 12582912, 14680064)),
 'blocks fp16 1 K=2': (41975808, (0, 2097152, 8388608, 10485760, 12582912, 14680064, 20971520, 23068672, 25165824, 27262976)),
 'blocks fp16 3 K=1': (88178688, (0, 6291456, 25165824, 31457280, 37748736, 44040192)),
 'blocks fp16 3 K=2': (125927424, (0, 6291456, 25165824, 31457280, 37748736, 44040192, 62914560, 69206016, 75497472, 81788928)),
 'blocks fp16 32 K=1': (940572672, (0, 67108864, 268435456, 335544320, 402653184, 469762048)),
 'blocks fp16 32 K=2': (1343225856, (0, 67108864, 268435456, 335544320, 402653184, 469762048, 671088640, 738197504, 805306368, 872415232)),
 'blocks fp32 1 K=1': (63963136, (0, 4194304, 16777216, 20971520, 25165824, 29360128)),
 'blocks fp32 1 K=2': (89128960, (0, 4194304, 16777216, 20971520, 25165824, 29360128, 41943040, 46137344, 50331648, 54525952)),
 'blocks fp32 3 K=1': (191889408, (0, 12582912, 50331648, 62914560, 75497472, 88080384)),
 'blocks fp32 3 K=2': (267386880, (0, 12582912, 50331648, 62914560, 75497472, 88080384, 125829120, 138412032, 150994944, 163577856)),
 'blocks fp32 32 K=1': (2046820352, (0, 134217728, 536870912, 671088640, 805306368, 939524096)),
 'blocks fp32 32 K=2': (2852126720, (0, 134217728, 536870912, 671088640, 805306368, 939524096, 1342177280, 1476395008, 1610612736, 1744830464)),
 'blocks pieces': (2, 12604416, (0, 1024, 2048, 3147776, 3150848, 3154944, 3159040, 4207616, 4208640, 4209664, 4210688, 8404992, 8409088, 12603392),
                   17694720, 524288),
 'dedup (1000, 37, 41)': 35072,
 'head_wgrad (1000, 448) (8192, 192) (1000, 100)': (924672, 3170304, 0),
 'invalid': (0, 0, 0, 0, 18446744073709551615, 18446744073709551615, 18446744073709551615, 0, 0, 0, 0, 0, 0),
 'label_stats (2, 256, 256, 6)': 5767680,
 'net bf16 1': (24150016, 23592960, 0, 2097152, (0, 524288, 1048576, 1572864), 16057344, (0, 1048576, 2097152, 3145728)),
 'net bf16 3': (72450048, 70778880, 0, 6291456, (0, 1572864, 3145728, 4718592), 43451392, (0, 3145728, 6291456, 9437184)),
 'net bf16 32': (772800512, 754974720, 0, 67108864, (0, 16777216, 33554432, 50331648), 440665088, (0, 33554432, 67108864, 100663296)),
 'net fp16 1': (24150016, 23592960, 0, 2097152, (0, 524288, 1048576, 1572864), 16057344, (0, 1048576, 2097152, 3145728)),
 'net fp16 3': (72450048, 70778880, 0, 6291456, (0, 1572864, 3145728, 4718592), 43451392, (0, 3145728, 6291456, 9437184)),
 'net fp16 32': (772800512, 754974720, 0, 67108864, (0, 16777216, 33554432, 50331648), 440665088, (0, 33554432, 67108864, 100663296)),
 'net fp32 1': (53477376, 42991616, 0, 13631488, (0, 1048576, 2097152, 3145728), 16057344, (0, 1048576, 2097152, 3145728)),
 'net fp32 3': (160432128, 128974848, 0, 40894464, (0, 3145728, 6291456, 9437184), 43451392, (0, 3145728, 6291456, 9437184)),
 'net fp32 32': (1711276032, 1375731712, 0, 436207616, (0, 33554432, 67108864, 100663296), 440665088, (0, 33554432, 67108864, 100663296)),
 'postproc (3, 224, 224)': 23142912,
 'pq (2, 256, 256, 6, 4096)': 787456,
 'unet bf16 1': (8291328, 22872064,
                 (0, 524288, 1048576, 1179648, 1310720, 1441792, 1507328, 1572864, 1638400, 1703936, 1769472, 1835008, 1900544, 1966080, 2031616,
                  2162688, 2686976, 3211264),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet bf16 3': (24478720, 51052544,
                 (0, 1572864, 3145728, 3538944, 3932160, 4325376, 4456448, 4587520, 4718592, 4784128, 4849664, 4915200, 5046272, 5177344, 5308416,
                  5701632, 7274496, 8847360),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet fp16 1': (8291328, 22872064,
                 (0, 524288, 1048576, 1179648, 1310720, 1441792, 1507328, 1572864, 1638400, 1703936, 1769472, 1835008, 1900544, 1966080, 2031616,
                  2162688, 2686976, 3211264),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet fp16 3': (24478720, 51052544,
                 (0, 1572864, 3145728, 3538944, 3932160, 4325376, 4456448, 4587520, 4718592, 4784128, 4849664, 4915200, 5046272, 5177344, 5308416,
                  5701632, 7274496, 8847360),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet fp32 1': (16581632, 22872064,
                 (0, 524288, 1048576, 1179648, 1310720, 1441792, 1507328, 1572864, 1638400, 1703936, 1769472, 1835008, 1900544, 1966080, 2031616,
                  2162688, 2686976, 3211264),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet fp32 3': (48956416, 51052544,
                 (0, 1572864, 3145728, 3538944, 3932160, 4325376, 4456448, 4587520, 4718592, 4784128, 4849664, 4915200, 5046272, 5177344, 5308416,
                  5701632, 7274496, 8847360),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 512, 512)),
 'unet params': (5256320,
                 (0, 295040, 368896, 401792, 475648, 623232, 688896, 836480, 984064, 1049728, 1197312, 1344896, 1410944, 1705984, 1779840, 1796480,
                  2386816, 4451712),
                 (294912, 368768, 401664, 475520, 623104, 688768, 836352, 983936, 1049600, 1197184, 1344768, 1410432, 1705856, 1779712, 1796224,
                  2386304, 4451200, 5254528),
                 (128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 512, 128, 128, 256, 512, 512, 1792),
                 (2304, 576, 256, 576, 1152, 512, 1152, 1152, 512, 1152, 1152, 128, 2304, 576, 64, 1152, 4032, 448))}


@pytest.fixture(scope="module")
def table():
    return layout_table(_lib.lib())


def test_every_query_is_pinned(table):
    assert sorted(table) == sorted(EXPECTED) and len(EXPECTED) == 9 + 1 + 6 + 4 + 1 + 18 + 3 + 1 + 1


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_layout_is_what_it_was(table, key):
    assert table[key] == EXPECTED[key]


def test_invalid_arguments_answer_zero_or_minus_one(table):
    inv = table["invalid"]
    assert inv[4:7] == (SIZE_MAX, SIZE_MAX, SIZE_MAX) and set(inv[:4] + inv[7:]) == {0}


def test_offsets_lie_inside_their_workspace_and_keep_256_byte_alignment(table):
    for name in DTYPES:
        for nS in (1, 3, 32):
            ws, neck, x, tr, fwd, bwd_bytes, bwd = table[f"net {name} {nS}"]
            es = 4 if name == "fp32" else 2
            assert x == 0 and neck % 256 == 0 and neck + nS * 1024 * 256 * es <= ws
            assert all(o % 256 == 0 and o + nS * 1024 * 256 * es <= tr for o in fwd) and list(fwd) == sorted(set(fwd))
            assert all(o % 256 == 0 and o + nS * 1024 * 256 * 4 <= bwd_bytes for o in bwd) and list(bwd) == sorted(set(bwd))


if __name__ == "__main__":
    import pprint
    lib = _lib._load(os.path.abspath(sys.argv[1]), _lib.SIGNATURES) if len(sys.argv) > 1 else _lib.lib()
    print("EXPECTED = " + pprint.pformat(layout_table(lib), width=150, compact=True))
