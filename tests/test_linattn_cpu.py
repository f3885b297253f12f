"""Linear attention (`use_linear_attn` / `attn_type="linear"`) without a GPU: the model classes construct with the
reference's parameter names, shapes, creation order and initial values (tests/golden/linattn_base.json, recorded from the
reference's own BaseVAE by make_golden_linattn.py), every other non-vanilla attention type still raises, and the new C
ABI entry points report argument errors without touching a device."""
import pytest
import torch

from golden_io import load_case

SMALL = dict(input_channels=1, latent_dim=4, hidden_channels=32, ch_mult=(1, 2), num_res_blocks=1,
             attn_resolutions=[14], dropout=0.0, resolution=28)


@pytest.mark.parametrize("switch", [dict(use_linear_attn=True), dict(attn_type="linear")], ids=["flag", "attn_type"])
def test_model_constructs_with_linear_attention(switch):
    import medvae_disentangled_multimodal_amd as M
    model = M.BaseVAE(**SMALL, **switch)
    blocks = [m for m in model.modules() if isinstance(m, M.LinAttnBlock)]
    assert len(blocks) == 5  # encoder level 1 + mid, decoder mid + the two blocks of level 1
    assert not any(isinstance(m, M.AttnBlock) for m in model.modules())
    for blk in blocks:
        assert blk.heads == 1 and blk.to_qkv.bias is None
        assert tuple(blk.to_qkv.weight.shape) == (192, 64, 1, 1) and tuple(blk.to_out.weight.shape) == (64, 64, 1, 1)


@pytest.mark.parametrize("cls,extra", [
    ("BetaVAE", dict(beta=4.0)),
    ("ConditionalVAE", dict(condition_method="concat")),
    ("DisentangledConditionalVAE", dict(num_modalities=5, shared_latent_dim=2, modality_latent_dim=2)),
])
def test_other_model_classes_pass_the_switch_through(cls, extra):
    import medvae_disentangled_multimodal_amd as M
    kw = {k: v for k, v in SMALL.items() if not (cls == "DisentangledConditionalVAE" and k in ("input_channels", "latent_dim"))}
    model = getattr(M, cls)(**kw, **extra, use_linear_attn=True)
    assert sum(isinstance(m, M.LinAttnBlock) for m in model.modules()) == 5
    enc = M.Encoder(ch=32, out_ch=1, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[14], in_channels=1,
                    resolution=28, z_channels=4, attn_type="linear")
    dec = M.Decoder(ch=32, out_ch=1, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[14], in_channels=1,
                    resolution=28, z_channels=4, use_linear_attn=True)
    assert isinstance(enc.mid.attn_1, M.LinAttnBlock) and isinstance(dec.up[1].attn[1], M.LinAttnBlock)


def test_state_dict_names_and_shapes_match_the_reference():
    import medvae_disentangled_multimodal_amd as M
    meta, _ = load_case("linattn_base")
    model = M.BaseVAE(**SMALL, use_linear_attn=True)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == meta["params"]  # same names, shapes and order
    assert sorted(got) == sorted(meta["params"])
    names = [k for k, _ in got]
    assert "encoder.mid.attn_1.to_qkv.weight" in names and "encoder.mid.attn_1.to_qkv.bias" not in names
    assert "decoder.up.1.attn.0.to_out.bias" in names


def test_seeded_initial_weights_match_the_reference():
    """torch.manual_seed(0): every tensor's (sum, sum of squares) equals the reference's -- the creation order
    (to_qkv, then to_out) and the bias-free to_qkv consume the RNG exactly as the reference does."""
    import medvae_disentangled_multimodal_amd as M
    meta, _ = load_case("linattn_base")
    torch.manual_seed(0)
    model = M.BaseVAE(**SMALL, use_linear_attn=True)
    ref = meta["seeded_init_torch_seed0"]
    sd = model.state_dict()
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        s, ss = float(v.double().sum()), float((v.double() ** 2).sum())
        assert abs(s - ref[k][0]) <= 1e-9 * max(1.0, abs(ref[k][0])), k
        assert abs(ss - ref[k][1]) <= 1e-9 * max(1.0, abs(ref[k][1])), k


def test_unknown_attention_type_still_raises():
    import medvae_disentangled_multimodal_amd as M
    from medvae_disentangled_multimodal_amd.encoder_decoder import make_attn
    with pytest.raises(NotImplementedError, match="bogus"):
        make_attn(64, "bogus")
    with pytest.raises(NotImplementedError, match="bogus"):
        M.BaseVAE(**SMALL, attn_type="bogus")
    assert isinstance(make_attn(64, "vanilla"), M.AttnBlock)


def test_multi_head_linear_attention_is_refused_clearly():
    import medvae_disentangled_multimodal_amd as M
    blk = M.LinearAttention(64)  # the reference's defaults: heads=4, dim_head=32
    assert tuple(blk.to_qkv.weight.shape) == (384, 64, 1, 1) and tuple(blk.to_out.weight.shape) == (64, 128, 1, 1)
    with pytest.raises(NotImplementedError, match="heads=4"):
        blk(torch.zeros(1, 64, 2, 2))


def test_linattn_entry_points_report_argument_errors_without_gpu():
    from medvae_disentangled_multimodal_amd import _lib
    lib = _lib.load()
    one = 16  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
    calls = [
        ("mvae_linattn_kstats", (None, 0, 0, None, 0, 0, 0, None, 0, None)),
        ("mvae_linattn_kstats", (one, 96, 96, one, 1, 0, 32, None, 0, None)),       # n = 0
        ("mvae_linattn_kstats", (one, 90, 90, one, 1, 1, 30, None, 0, None)),       # c % 4
        ("mvae_linattn_kstats", (one, 16, 16, one, 1, 1, 32, None, 0, None)),       # ld < c
        ("mvae_linattn_kstats", (one, 96, 96, None, 1, 1, 32, None, 0, None)),      # no stats
        ("mvae_linattn_ksoftmax", (None, 0, 0, None, None, 0, 0, 0, None)),
        ("mvae_linattn_ksoftmax", (one, 96, 96, one, None, 1, 1, 32, None)),        # no output
        ("mvae_linattn_dk", (None, 0, 0, None, None, 0, 0, 0, 0, 0, None, 0, None)),
        ("mvae_linattn_dk", (one, 96, 96, one, one, 8, 96, 1, 1, 32, None, 0, None)),  # lddk < c
    ]
    for name, args in calls:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert b"linattn" in lib.mvae_last_error(), (name, lib.mvae_last_error())
    assert getattr(lib, "mvae_linattn_kstats")(one, 90, 90, one, 1, 1, 30, None, 0, None) == -1
    assert b"c = 30" in lib.mvae_last_error()
    with pytest.raises(RuntimeError, match="linattn"):
        _lib.call("mvae_linattn_ksoftmax", None, 0, 0, None, None, 0, 0, 0, None)
    # a missing workspace is reported too (status -2, like the other workspace-taking entry points)
    assert lib.mvae_linattn_dk(one, 96, 96, one, one, 96, 96, 1, 1, 32, None, 0, None) == -2
    assert b"linattn" in lib.mvae_last_error()
    # host-side planning: the statistics of 784 tokens are split across workgroups, one token is not
    assert _lib.query("mvae_linattn_workspace_bytes", 2, 784, 128) > 2 * 2 * 128 * 4
    assert _lib.query("mvae_linattn_workspace_bytes", 2, 1, 32) == 2 * 32 * 4
    assert _lib.query("mvae_linattn_workspace_bytes", 0, 0, 0) == 0
