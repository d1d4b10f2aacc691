"""CPU: which 3x3 launches take the persistent output convolution (ops.out_walk_bank / ops.out_walk_selected, applied by
ops.pack_conv_weight and ops.conv2d), with the library mocked so that every pack and launch is only recorded; and the kernel's
host-side geometry (csrc/conv_split_out_geom.h) in a stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, SPLIT, FP32 = "cwfa_conv3x3_out_split_f32", "cwfa_conv3x3_split_f32", "cwfa_conv2d_f32"


class FakeLib:
    """stands in for libcwfa_hip.so: every entry point returns success and is recorded; the *_packed_* sizes are small numbers"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            if name == "cwfa_conv3x3_out_split_packed_bytes":
                return 18 * 3 * 4 * 16 * ((a[0] + 15) // 16) * 16
            return 64 if "packed" in name else 0
        return f


@pytest.fixture
def fake(monkeypatch):
    from cwfa_amd import ops
    lib = FakeLib()
    monkeypatch.setattr(ops._lib, "lib", lambda: lib)
    monkeypatch.setattr(ops, "_dev", lambda t, name="tensor": t)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    for k in ("_split_bf16", "_precision", "_pack_epoch", "OUT_WALK", "OUT_WALK_MT", "conv_event_sink"):
        monkeypatch.setattr(ops, k, getattr(ops, k))          # restored after the test
    ops.OUT_WALK, ops.OUT_WALK_MT, ops.conv_event_sink = True, (1, 2, 3), None
    return lib


def run(ops, lib, cin, cout, **kw):
    """pack a [cout, cin, 3, 3] bank and launch it on a 1 x cin x 8 x 8 input; -> (the pack calls, the convolution launched)"""
    del lib.calls[:]
    pc = ops.pack_conv_weight(torch.zeros(cout, cin, 3, 3))
    packs = [c for c in lib.calls if c.endswith("_pack_f32")]
    del lib.calls[:]
    ops.conv2d(torch.zeros(1, cin, 8, 8), pc, bias=torch.zeros(cout), **kw)
    launches = [c for c in lib.calls if c.startswith("cwfa_conv")]       # (a narrow bank's load-side prologue is a pass of its own)
    assert len(launches) == 1, launches
    return packs, launches[0]


@pytest.mark.parametrize("mode", ("split_bf16", "bf16", "fp16"))
def test_rule_boundaries(fake, mode):
    from cwfa_amd import ops
    ops.set_precision(mode)
    for cout in (1, 12, 16, 17, 24, 32, 33, 48):
        packs, launch = run(ops, fake, 64, cout)
        assert "cwfa_conv3x3_out_split_pack_f32" in packs and launch == OUT, (cout, packs, launch)
    # the bank: exactly 64 inputs, at most 48 outputs
    assert run(ops, fake, 63, 48) == (["cwfa_conv3x3_split_pack_f32"], SPLIT)
    assert run(ops, fake, 64, 49) == (["cwfa_conv3x3_split_pack_f32"], SPLIT)
    assert run(ops, fake, 29, 12)[1] == SPLIT                                  # the condition nets' banks
    assert run(ops, fake, 64, 96)[1] == SPLIT
    # the call: bias only, nothing on the load side, NCHW output, no statistics -- anything else keeps the bank's other image
    sc, sh = torch.ones(64), torch.zeros(64)
    assert run(ops, fake, 64, 48, in_scale=sc, in_shift=sh)[1] == SPLIT
    assert run(ops, fake, 64, 48, in_add=torch.zeros(1, 64, 8, 8))[1] == SPLIT
    assert run(ops, fake, 64, 48, act="elu")[1] == SPLIT
    assert run(ops, fake, 64, 48, act="prelu", prelu_alpha=torch.ones(1))[1] == SPLIT
    assert run(ops, fake, 64, 48, residual=torch.zeros(1, 48, 8, 8))[1] == SPLIT
    # blocked input is accepted where the kernel is selected, also for a bank whose other image is an fp32 one
    assert run(ops, fake, 64, 48, in_blocked=True)[1] == OUT


def test_rule_function_alone(fake):
    """the launch-side conditions conv2d cannot be driven into without device tensors: statistics, blocked output, a second source,
    an image beyond 32-bit byte offsets"""
    from cwfa_amd import ops
    ops.set_precision("split_bf16")
    pc = ops.pack_conv_weight(torch.zeros(48, 64, 3, 3))
    assert ops.out_walk_selected(pc, 8, 8) and not ops.out_walk_selected(pc, 8, 8, out_stats=object())
    assert not ops.out_walk_selected(pc, 8, 8, out_blocked=True) and not ops.out_walk_selected(pc, 8, 8, cat=object())
    assert not ops.out_walk_selected(pc, 4096, 4096)                          # 64 planes beyond 32-bit byte offsets


def test_fp32_precision_and_switch(fake):
    from cwfa_amd import ops
    ops.set_precision("fp32")
    for cout in (12, 24, 48):
        assert run(ops, fake, 64, cout) == (["cwfa_conv2d_pack_f32"], FP32)
    ops.set_precision("split_bf16")
    today = {}
    ops.OUT_WALK = False                          # the switch off: today's dispatch, for every width
    for cout in (12, 24, 48):
        today[cout] = run(ops, fake, 64, cout)
    assert today == {12: (["cwfa_conv3x3_split_pack_f32"], SPLIT), 24: (["cwfa_conv2d_pack_f32"], FP32), 48: (["cwfa_conv3x3_split_pack_f32"], SPLIT)}
    ops.OUT_WALK = True
    pc = ops.pack_conv_weight(torch.zeros(12, 64, 3, 3))
    assert pc.walk is not None and pc.split
    ops.OUT_WALK = False                          # off at launch time too: a bank packed with the switch on takes its other image
    del fake.calls[:]
    ops.conv2d(torch.zeros(1, 64, 8, 8), pc, bias=torch.zeros(12))
    assert fake.calls == [SPLIT]
    ops.OUT_WALK = True
    # a width sent back by the per-width decision keeps today's kernel
    ops.OUT_WALK_MT = (1, 3)
    assert run(ops, fake, 64, 24) == today[24] and run(ops, fake, 64, 12)[1] == OUT and run(ops, fake, 64, 48)[1] == OUT


def test_subnetwork_keeps_blocked_maps_for_the_selected_bank(fake):
    """networks._stack asks the same rule whether the last layer may leave its map channel-blocked"""
    from cwfa_amd import ops
    ops.set_precision("split_bf16")
    pc24 = ops.pack_conv_weight(torch.zeros(24, 64, 3, 3))
    assert not pc24.split and ops.out_walk_selected(pc24, 512, 512)
    ops.OUT_WALK = False
    assert not ops.out_walk_selected(pc24, 512, 512)


def test_host_geometry_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "split_out_geom")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "cwfa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "split_out_geom_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "split_out_geom: ok" in r.stdout, r.stdout + r.stderr
