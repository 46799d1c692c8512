"""The MFM fusion for clips of 9 - 16 frames, host side (no GPU): the library exports the three entry points of the 16-token
attention family under the unchanged ABI version and checks its shapes before any HIP call, the fusions refuse 17 frames before any kernel
runs, and the two command lines that build a fusion refuse a --seq_len beyond 16."""
import argparse
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"lmkd_mha_seq": 7, "lmkd_mha_seq_train_fwd": 9, "lmkd_mha_seq_bwd": 10}
EINVAL = -1


def test_library_exports_the_entry_points_under_abi_3():
    import litemkd_amd
    L = litemkd_amd.lib()
    assert L.value("lmkd_abi_version") == 3
    text = open(os.path.join(ROOT, "include", "lmkd.h")).read()
    assert re.search(r"^#define\s+LMKD_MHA_SEQ_MAX_L\s+16\s*$", text, flags=re.M)
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(L.cdll, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(L.protos[name][1]) == nargs, name
    from litemkd_amd import ops
    assert ops.MFM_MAX_L == 16


def test_shapes_are_checked_before_any_hip_call():
    """null buffers and no GPU: the checks come first, so these return the invalid-argument code instead of touching the device"""
    import litemkd_amd
    lib = litemkd_amd.lib()
    c = lib.cdll

    def attn(B, L, D, H, expect):
        got = []
        for call in (lambda: c.lmkd_mha_seq(None, None, B, L, D, H, None),
                     lambda: c.lmkd_mha_seq_train_fwd(None, None, None, None, B, L, D, H, None),
                     lambda: c.lmkd_mha_seq_bwd(None, None, None, None, None, B, L, D, H, None)):
            got.append((call(), lib.last_error()))
        assert all(rc == EINVAL for rc, _ in got), (B, L, D, H, got)
        assert all(expect in msg for _, msg in got), (expect, got)
        assert [msg.split(":")[0] for _, msg in got] == list(ENTRY_POINTS), got      # each names itself
    attn(0, 12, 128, 2, "0 sequences")
    attn(2, 12, 128, 0, "0 heads")
    attn(2, 0, 128, 2, "0 tokens")
    attn(2, 17, 128, 2, "17 tokens")
    attn(2, 12, 130, 4, "width 130 is no multiple of 4 heads")
    attn(2, 9, 128, 2, "null pointer")      # the shapes pass and the null buffers are what is refused
    attn(2, 16, 128, 2, "null pointer")


def test_attention_family_by_length():
    from litemkd_amd import ops
    assert [ops.mfm_attn_family(L) for L in (1, 8, 9, 16)] == [("small", 8), ("small", 8), ("seq", 16), ("seq", 16)]
    with pytest.raises(RuntimeError, match="16"):
        ops.mfm_attn_family(17)


@pytest.mark.parametrize("n_mod", [2, 3])
def test_fusions_refuse_17_frames_before_any_kernel(n_mod):
    from litemkd_amd.teacher.mfm import ThreeTransforTemproal, TwoTransforFusion
    cls = ThreeTransforTemproal if n_mod == 3 else TwoTransforFusion
    m = cls(argparse.Namespace(seq_len=17, trans_num=1), in_channels=64).eval()
    xs = [torch.zeros(2, 17, 64) for _ in range(n_mod)]      # CPU tensors: a kernel launch on them would fail otherwise
    for fn in (m.forward, m.extract_feature):
        with pytest.raises(ValueError, match=r"features \(2, 17, 64\): the fusion takes \[N, L <= 16, 64\]"):
            fn(*xs)
    with pytest.raises(ValueError, match=r"L <= 16, 64"):      # the width is part of the same check
        m.extract_feature(*[torch.zeros(2, 12, 32) for _ in range(n_mod)])


def test_command_lines_refuse_a_seq_len_beyond_16(capsys):
    from litemkd_amd import extract as EX
    from litemkd_amd import train_teacher as TT
    p = TT.build_parser()
    ok = "--synthetic --no_save".split()
    for L in (1, 12, 16):
        assert TT.args_check(p, p.parse_args(ok + ["--seq_len", str(L), "--shirt_num", "0"])).seq_len == L
    assert TT.args_check(p, p.parse_args(ok + ["--seq_len", "12", "--shirt_num", "11"])).shirt_num == 11
    for bad, text in ((["--seq_len", "17"], "--seq_len 17"), (["--seq_len", "0", "--shirt_num", "0"], "--seq_len 0"),
                      (["--seq_len", "12", "--shirt_num", "12"], "--shirt_num 12")):
        with pytest.raises(SystemExit):
            TT.args_check(p, p.parse_args(ok + bad))
        assert text in capsys.readouterr().err
    e = EX.build_parser()
    fusion = "--stage fusion --out o --feature_save_path f --checkpoint_dir c.pt".split()
    assert EX.args_check(e, e.parse_args(fusion + ["--seq_len", "16"])).seq_len == 16
    with pytest.raises(SystemExit):
        EX.args_check(e, e.parse_args(fusion + ["--seq_len", "17"]))
    assert "--seq_len 17" in capsys.readouterr().err
    # the trunk of --stage modality takes any number of frames
    modality = "--stage modality --out o --path p --traintestlist l --init_weights w.pt".split()
    assert EX.args_check(e, e.parse_args(modality + ["--seq_len", "17"])).seq_len == 17
