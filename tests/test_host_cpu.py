"""CPU-only checks of the product's host logic: registries and their error behaviour, schedule
tables (bit-exact vs the reference-captured golden), string-valued config parsing, state_dict
layout, the C-ABI library's exported symbols, and the loud failure without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import unet_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import posterior_mean_variance as pmv  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402
from osmosis_diffusion_code_amd.osmosis_utils import utils as utilso  # noqa: E402
from osmosis_diffusion_code_amd.osmosis_utils import losses as losseso  # noqa: E402
from osmosis_diffusion_code_amd import _lib  # noqa: E402

DIFF = dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
            model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False,
            rescale_timesteps=False)


@pytest.mark.parametrize("tag,resp", [("T1000", 1000), ("T250", "250"), ("T10", [10])])
def test_sampler_tables_bit_exact_vs_reference(tag, resp):
    g = dict(np.load(os.path.join(GOLD, "schedules.npz")))
    s = gd.create_sampler(timestep_respacing=resp, **DIFF)
    assert np.array_equal(s.betas, g[f"{tag}.betas"])
    assert s.timestep_map == list(g[f"{tag}.timestep_map"])
    assert np.array_equal(s.mean_processor.sqrt_recip_alphas_cumprod, g[f"{tag}.sqrt_recip_alphas_cumprod"])
    assert np.array_equal(s.mean_processor.sqrt_recipm1_alphas_cumprod, g[f"{tag}.sqrt_recipm1_alphas_cumprod"])
    assert np.array_equal(s.mean_processor.posterior_mean_coef1, g[f"{tag}.posterior_mean_coef1"])
    assert np.array_equal(s.mean_processor.posterior_mean_coef2, g[f"{tag}.posterior_mean_coef2"])
    assert np.array_equal(s.var_processor.posterior_log_variance_clipped, g[f"{tag}.posterior_log_variance_clipped"])
    tab = s.coef_table()
    T = s.num_timesteps
    assert tab.shape == (T, 8) and tab.dtype == np.float32
    assert np.array_equal(tab[:, 0], g[f"{tag}.sqrt_recip_alphas_cumprod"].astype(np.float32))
    assert np.array_equal(tab[:, 5], g[f"{tag}.log_betas"].astype(np.float32))
    assert tab[0, 6] == 0.0 and (tab[1:, 6] == 1.0).all()
    assert np.array_equal(tab[:, 7], np.array(s.timestep_map, dtype=np.float32))


def test_schedule_helpers_and_errors():
    g = dict(np.load(os.path.join(GOLD, "schedules.npz")))
    assert np.array_equal(gd.get_named_beta_schedule("cosine", 50), g["cosine50.betas"])
    assert sorted(gd.space_timesteps(300, [10, 15, 20])) == list(g["space_1000_10_15_20"])
    assert sorted(gd.space_timesteps(1000, "ddim25")) == list(g["space_ddim25"])
    with pytest.raises(NotImplementedError):
        gd.get_named_beta_schedule("quadratic", 10)
    with pytest.raises(ValueError):
        gd.space_timesteps(10, [20])
    with pytest.raises(ValueError):
        gd.space_timesteps(1000, "ddim999")


def test_registries_raise_like_the_reference():
    with pytest.raises(NameError):
        gd.get_sampler("nope")
    with pytest.raises(NameError):
        gd.register_sampler("ddpm")(object)
    with pytest.raises(NameError):
        M.get_operator("nope", device="cpu")
    with pytest.raises(NameError):
        M.register_operator("haze_physical")(object)
    with pytest.raises(NameError):
        M.get_noise("nope")
    with pytest.raises(NameError):
        CM.get_conditioning_method("nope", None, None)
    with pytest.raises(NameError):
        CM.register_conditioning_method("osmosis")(object)
    with pytest.raises(NameError):
        pmv.get_mean_processor("nope", betas=None, dynamic_threshold=False, clip_denoised=False)
    with pytest.raises(NameError):
        pmv.get_var_processor("nope", betas=None)
    with pytest.raises(NameError):
        losseso.get_loss("nope")
    # third-party additions stay possible
    @M.register_noise("unit_test_noise")
    class _N(M.Noise):
        def forward(self, data):
            return data
    assert M.get_noise("unit_test_noise").__name__ == "unit_test_noise"


def test_operator_config_parsing():
    op = M.get_operator("underwater_physical_revised", device="cpu", batch_size=2, optimizer="sgd",
                        depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_a_eta="1e-5",
                        phi_b="0.95, 0.8, 0.8", phi_b_learn_flag=False, phi_inf="0.14, 0.29, 0.49")
    assert op.__name__ == "underwater_physical_revised"
    assert op.phi.shape == (2, 9)
    assert np.allclose(op.phi[1].numpy(), [1.1, 0.95, 0.95, 0.95, 0.8, 0.8, 0.14, 0.29, 0.49])
    assert op.eta3() == (1e-5, 0.0, 1e-5)
    v = op.variables()
    assert set(v) == {"phi_a", "phi_b", "phi_inf"} and v["phi_a"].shape == (2, 3, 1, 1)
    hz = M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", depth_type="gamma",
                        value="1.4,1.4,1", optimizer="GD")
    assert hz.variables()["phi_ab"].shape == (1, 1, 1, 1)
    assert M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", optimizer="Adam").optimizer == "adam"
    assert M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", optimizer="RMSprop").optimizer == "rmsprop"
    with pytest.raises(NotImplementedError):       # utils.get_optimizer's two names that cannot step phi in the reference either
        M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", optimizer="lbfgs")
    with pytest.raises(ValueError):
        M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", optimizer="bogus")
    with pytest.raises(NotImplementedError):
        M.get_operator("haze_physical", device="cpu", phi_ab="1.0", phi_inf="0.1,0.2,0.3", depth_type="cubic")
    # forward model on CPU tensors == oracle formula
    from oracle.diffusion_ref import PhysOperator
    ref = PhysOperator("haze_physical", depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_inf="0.1,0.2,0.3")
    x = torch.randn(1, 4, 5, 5, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(hz.forward(x), ref.forward(x), atol=1e-7)


def test_conditioning_config_parsing():
    op = M.get_operator("underwater_physical", device="cpu", phi_ab="1,1,1", phi_inf="0.2,0.4,0.7", optimizer="sgd")
    c = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), scale="7,7,7,0.9",
                                   gradient_clip="True,0.005", gradient_x_prev=True, n_iter=20,
                                   aux_loss={"avrg_loss": 0.5, "val_loss": "20"}, weight_function="gamma,1.4,1.4,1",
                                   loss_weight="depth")
    assert c.scale.tolist() == pytest.approx([7, 7, 7, 0.9])
    assert c.gradient_clip and c.gradient_clip_value == 0.005 and c.n_iter == 20
    assert c.aux_loss.kernel_coefficients() == {"gamma_avrg": 0.5, "gamma_val": 20.0}
    c2 = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), scale=3.0, gradient_clip="False")
    assert c2.scale.tolist() == [3.0] and not c2.gradient_clip and c2.clip_value == -1.0
    assert utilso.parse_weight_function("gamma,1.4,1.4,1")[0] == "gamma"
    assert utilso.str2bool("Yes") and not utilso.str2bool("0")
    with pytest.raises(Exception):
        utilso.str2bool("maybe")


def test_freeze_and_alternate_schedule():
    p = dict(pattern="pcgs", update_start=0.7, update_end=0, s_start=1, s_end=0, local_M=1,
             start_guidance=1, stop_guidance=0)
    assert utilso.is_freeze_phi(p, 999, 1000) and utilso.is_freeze_phi(p, 701, 1000)
    assert not utilso.is_freeze_phi(p, 700, 1000) and not utilso.is_freeze_phi(p, 0, 1000)
    assert not utilso.is_freeze_phi({"pattern": "original"}, 5, 10) and not utilso.is_freeze_phi(None, 5, 10)
    assert utilso.set_alternate_length(p, 500, 1000) == 1
    from oracle.diffusion_ref import is_freeze_phi as ref_freeze
    for idx in range(0, 1000, 37):
        assert utilso.is_freeze_phi(p, idx, 1000) == ref_freeze(p, idx, 1000)


def test_state_dict_layout_matches_reference_keys():
    kw = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2",
              attention_resolutions="128,64", num_head_channels=16, num_heads=4, learn_sigma=True,
              use_scale_shift_norm=True, resblock_updown=True, pretrain_model="osmosis")
    m = unet.create_model(**kw)
    shapes = U.param_shapes(U.UNetConfig.from_create_model_kwargs(**kw))
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k], k
    # same key set as the golden blocks captured from the reference modules
    g = np.load(os.path.join(GOLD, "blocks.npz"))
    ref_keys = {k.split(".sd.")[1] for k in g.files if k.startswith("res_skip.sd.")}
    ours = {k[len("input_blocks.3.0."):] for k in sd if k.startswith("input_blocks.3.0.")}
    assert ours == ref_keys
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 32, 32), torch.zeros(1))


def test_full_size_model_has_the_reference_parameter_count():
    cfg = U.UNetConfig.from_create_model_kwargs(image_size=256, num_channels=256, num_res_blocks=2,
                                                attention_resolutions="32, 16, 8", num_heads=4,
                                                num_head_channels=64, use_scale_shift_norm=True,
                                                resblock_updown=True, learn_sigma=True, pretrain_model="osmosis")
    n = sum(int(np.prod(s)) for s in U.param_shapes(cfg).values())
    assert n == 552_821_000   # SURVEY.md section 6 [probe]


def test_create_model_argument_errors():
    with pytest.raises(ValueError):
        unet.create_model(image_size=100, num_channels=32, num_res_blocks=1)
    with pytest.raises(NotImplementedError):
        unet.create_model(image_size=64, num_channels=32, num_res_blocks=1, attention_resolutions=1.5)


def test_product_path_fails_loudly_on_cpu_tensors():
    from osmosis_diffusion_code_amd import ops
    with pytest.raises(_lib.OsmosisHipError, match="no CPU fallback"):
        ops.timestep_embedding(torch.zeros(2), torch.zeros(2, 8), 2, 8)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "osmosis_diffusion_code_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(dp, f)


def test_create_model_loads_a_checkpoint_file_and_survives_a_bad_path(tmp_path, capsys, monkeypatch):
    """N4 / unet.py:86-97: `model_path` is th.load-ed into the module (reference keys, OIHW shapes); any failure is
    caught, reported as 'Got exception: ... / Randomly initialize', and the model is still returned."""
    from oracle import unet_ref as U
    from osmosis_diffusion_code_amd.guided_diffusion import unet
    kw = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
              num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
              pretrain_model="osmosis")
    sd = U.seeded_state_dict(U.UNetConfig.from_create_model_kwargs(**kw), 77)
    path = tmp_path / "ckpt.pt"
    torch.save(sd, path)
    m = unet.create_model(model_path=str(path), **kw)
    assert "Got exception" not in capsys.readouterr().out
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    m2 = unet.create_model(model_path=str(tmp_path / "missing.pt"), **kw)
    assert "Got exception" in capsys.readouterr().out          # message printed, nothing raised
    assert set(m2.state_dict()) == set(sd)
    # strict mode (SURVEY section 5 / VERDICT r04 item 8): the same failures RAISE -- a missing file, and a file of another architecture
    with pytest.raises(RuntimeError, match="could not be loaded"):
        unet.create_model(model_path=str(tmp_path / "missing.pt"), strict_checkpoint=True, **kw)
    wrong = {k: v for k, v in sd.items() if not k.startswith("out.")}
    torch.save(wrong, tmp_path / "wrong.pt")
    with pytest.raises(RuntimeError, match="could not be loaded"):
        unet.create_model(model_path=str(tmp_path / "wrong.pt"), strict_checkpoint=True, **kw)
    monkeypatch.setenv("OSM_STRICT_CHECKPOINT", "1")
    with pytest.raises(RuntimeError):
        unet.create_model(model_path=str(tmp_path / "missing.pt"), **kw)
    unet.create_model(model_path=str(path), **kw)                # a good checkpoint loads in strict mode
    monkeypatch.setenv("OSM_STRICT_CHECKPOINT", "0")
    unet.create_model(model_path=str(tmp_path / "missing.pt"), **kw)


def test_c_abi_header_is_plain_c_and_links_from_c(tmp_path):
    """The drop-in boundary is a C ABI: include/osmosis_hip.h compiles as strict C99 and a C program linked against
    libosmosis_hip.so can call it (entry points that need no GPU: version, argument validation, shape queries)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "osmosis_diffusion_code_amd")
    exe = str(tmp_path / "c_abi_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
           os.path.join(root, "examples", "c_abi_check.c"), "-L", libdir, "-losmosis_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rc -1" in run.stdout and "null pointer" in run.stdout


def test_poisson_and_gaussian_noisers_follow_the_reference_recipe():
    """measurements.py:471-507: gaussian adds sigma * randn; poisson draws np.random.poisson(255 * rate * img01) and maps
    back to [-1, 1] (seeded numpy stream, clamped)."""
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    x = torch.linspace(-1, 1, 3 * 8 * 8).reshape(1, 3, 8, 8)
    torch.manual_seed(5)
    y = M.get_noise("gaussian", sigma=0.1)(x)
    torch.manual_seed(5)
    assert torch.allclose(y, x + 0.1 * torch.randn_like(x))
    np.random.seed(3)
    yp = M.get_noise("poisson", rate=1.0)(x)
    np.random.seed(3)
    d01 = ((x + 1.0) / 2.0).clamp(0, 1)
    want = (torch.from_numpy(np.random.poisson(d01 * 255.0 * 1.0) / 255.0 / 1.0) * 2.0 - 1.0).clamp(-1, 1)
    assert torch.equal(yp, want) and float(yp.min()) >= -1 and float(yp.max()) <= 1
    assert M.get_noise("clean")(x) is x
    with pytest.raises(NameError):
        M.get_noise("salt")


def test_process_grid_layout(tmp_path):
    """`<name>_process.png` of the fused loop's recording (gaussian_diffusion.py:308-333): RGB row over depth row, one column
    per snapshot, 2-pixel padding like torchvision.utils.make_grid."""
    from PIL import Image
    from osmosis_diffusion_code_amd.guided_diffusion.gaussian_diffusion import GaussianDiffusion
    g = torch.Generator().manual_seed(0)
    recs = [(idx, torch.rand(1, 4, 16, 12, generator=g) * 2 - 1) for idx in (999, 800, 0)]
    path = GaussianDiffusion._save_process_grid(recs, str(tmp_path), "img7")
    assert path.endswith("img7_process.png")
    im = np.asarray(Image.open(path))
    assert im.shape == (2 * (16 + 2) + 2, 3 * (12 + 2) + 2, 3)
    assert (im[:2] == 0).all() and (im[:, :2] == 0).all()          # padding
    # tvtf.to_pil_image (the reference's writer, gaussian_diffusion.py:332) truncates: pic.mul(255).byte()
    want = torch.clamp(0.5 * (recs[1][1][0, 0:3] + 1), 0, 1).mul(255).to(torch.uint8)
    assert np.array_equal(im[2:18, 2 + 14:2 + 14 + 12], want.permute(1, 2, 0).numpy())
    assert GaussianDiffusion._save_process_grid(recs, None, "x") is None


def test_activation_footprint_estimate_and_architecture_walk():
    """engine.describe_architecture / activation_bytes_per_image (sizes batches per pass): shapes-only, no device."""
    import contextlib
    import io
    from osmosis_diffusion_code_amd.engine import activation_bytes_per_image, describe_architecture
    from osmosis_diffusion_code_amd.guided_diffusion import unet
    with contextlib.redirect_stdout(io.StringIO()):
        m = unet.create_model(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2",
                              attention_resolutions="128,64", num_head_channels=16, num_heads=4, learn_sigma=True,
                              use_scale_shift_norm=True, resblock_updown=True, pretrain_model="osmosis")
    a = describe_architecture(m)
    assert a["cin"] == 4 and a["cout"] == 8 and a["inp"][0] == [("conv", 4, 32)]
    assert [l[0] for l in a["mid"]] == ["res", "attn", "res"]
    # channel_mult 1,2,2 with attention at ds 2 and 4: 2 input + 1 middle + 4 output attention blocks
    assert sum(1 for s in a["inp"] + a["outb"] + [a["mid"]] for l in s if l[0] == "attn") == 7
    b32 = activation_bytes_per_image(a, 32, 32, 4)
    b64 = activation_bytes_per_image(a, 64, 64, 4)
    h64 = activation_bytes_per_image(a, 64, 64, 2)
    assert 3.0 < (b64 - 16 * 2 ** 20) / (b32 - 16 * 2 ** 20) < 17.0     # 4x the pixels, 16x the T^2 attention terms
    assert h64 < b64


def test_fused_loop_argument_checks_need_no_gpu():
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.osmosis_utils.diffusion import GaussianDiffusion as Prior
    c = CM.PosteriorSamplingOsmosis(operator=None, noiser=None, scale="7,7,7,0.9", gradient_x_prev=False,
                                    gradient_clip="True,0.005")
    assert c.gradient_clip and c.clip_value == -1.0      # the x0-gradient branch of the reference is not clipped (:222-224)
    c0 = CM.PosteriorSamplingOsmosis(operator=None, noiser=None, scale="1", gradient_x_prev=True, gradient_clip="True,0")
    assert c0.clip_value == 0.0                           # clamp to zero, like torch.clamp(g, -0, 0)
    with pytest.raises(NotImplementedError):              # inverse() drives the HIP UNetModel only
        Prior(1000, "linear").inverse(object(), shape=(4, 8, 8), steps=5, start_t=3)


def test_chunk_sizes_of_a_batch_that_does_not_fit():
    """GaussianDiffusion.chunk_sizes: fewest chunks, at most two sizes (an engine per size owns its activations, so the two
    sizes together must fit the cap); a prime batch above the cap no longer degenerates into chunks of one image."""
    from osmosis_diffusion_code_amd.guided_diffusion.gaussian_diffusion import GaussianDiffusion as GD
    assert GD.chunk_sizes(32, 32) == [32] and GD.chunk_sizes(32, 100) == [32]
    assert GD.chunk_sizes(32, 16) == [16, 16]
    assert GD.chunk_sizes(37, 32) == [13, 12, 12]
    assert GD.chunk_sizes(33, 32) == [11, 11, 11]
    assert GD.chunk_sizes(5, 4) == [2, 2, 1]
    assert GD.chunk_sizes(3, 2) == [1, 1, 1] and GD.chunk_sizes(7, 1) == [1] * 7
    for B in range(1, 80):
        for cap in range(1, 40):
            sz = GD.chunk_sizes(B, cap)
            kinds = sorted(set(sz))
            assert sum(sz) == B and max(sz) <= cap and len(kinds) <= 2
            assert len(kinds) == 1 or sum(kinds) <= cap
            assert sz == sorted(sz, reverse=True)


def test_xmax_registry_forgets_a_bound_when_someone_else_writes_the_buffer():
    """the f16x3 range hand-over (`max |dy| was left behind by the pass that wrote dy`) must not survive
    another writer of the same memory.  The registry logic needs no device: matrices over CPU tensors."""
    from osmosis_diffusion_code_amd.engine import UNetEngine
    from osmosis_diffusion_code_amd.ops import Mat
    eng = UNetEngine.__new__(UNetEngine)
    eng._xmax_reg = {}
    buf = torch.zeros(64, 48)
    other = torch.zeros(64, 48)
    full, left, right = Mat.of(buf), Mat.of(buf).cols_slice(0, 16), Mat.of(buf).cols_slice(16, 48)
    slot = torch.zeros(4)
    eng._xmax_register(full, slot)
    assert eng._xmax_lookup(full) is slot
    assert eng._xmax_lookup(left) is slot              # the left column slice shares (pointer, rows, ld): the wider bound serves it
    assert eng._xmax_lookup(right) is None and eng._xmax_lookup(Mat.of(other)) is None
    eng._xmax_invalidate(Mat.of(other))                # a write elsewhere changes nothing
    assert eng._xmax_lookup(full) is slot
    eng._xmax_invalidate(right)                        # a write into a column slice of the buffer drops the bound over it
    assert eng._xmax_lookup(full) is None and eng._xmax_lookup(left) is None
    slot2 = torch.zeros(4)
    eng._xmax_register(full, slot)
    eng._xmax_register(right, slot2)                   # registering a slice replaces whatever covered that memory
    assert eng._xmax_lookup(full) is None and eng._xmax_lookup(right) is slot2


def test_unet_variants_have_the_reference_keys_and_a_memory_estimate():
    """Round 5: every UNetModel option create_model can reach builds (Upsample / Downsample layers with or without a convolution,
    additive conditioning, class conditioning, dropout accepted and inert); state_dict keys / shapes equal the oracle's list (which
    gen_golden.py loads strictly into the REAL reference module); the dry-run activation estimate covers the new layer kinds."""
    from osmosis_diffusion_code_amd.engine import activation_bytes_per_image, describe_architecture
    from osmosis_diffusion_code_amd.guided_diffusion.unet import UNetModel
    base = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
                num_head_channels=16, num_heads=4, learn_sigma=True, pretrain_model="osmosis")
    for extra in (dict(resblock_updown=False, use_scale_shift_norm=False), dict(resblock_updown=False, use_scale_shift_norm=True,
                  class_cond=True, dropout=0.1), dict(resblock_updown=True, use_scale_shift_norm=False), dict()):
        kw = dict(base, **extra)
        m = unet.create_model(**kw)
        want = U.param_shapes(U.UNetConfig.from_create_model_kwargs(**kw))
        got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert got == want, (extra, set(got) ^ set(want))
        assert activation_bytes_per_image(describe_architecture(m), 64, 64) > 0
    m = UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,),
                  channel_mult=(1, 2), conv_resample=False, num_head_channels=16)       # conv-less resampling layers: no parameters
    assert not any(".op." in k or k.endswith(".conv.weight") for k in m.state_dict())
    with pytest.raises(NotImplementedError):
        UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,), dims=3)


def test_recorder_suspended_runs_now_and_records_nothing():
    """One-off work triggered while a launch plan is being recorded (a weight image packed on first use, engine._Conv.direct_f16x3)
    must not become part of the plan: Recorder.suspended() hides the active recorders and restores them, also on an exception."""
    from osmosis_diffusion_code_amd import _lib
    with _lib.Recorder() as outer:
        assert _lib._state.recorders == [outer]
        with _lib.Recorder.suspended():
            assert _lib._state.recorders == []
            with _lib.Recorder() as inner:          # a recorder opened inside is the only one that sees calls
                assert _lib._state.recorders == [inner]
            assert _lib._state.recorders == []
        assert _lib._state.recorders == [outer]
        with pytest.raises(RuntimeError):
            with _lib.Recorder.suspended():
                raise RuntimeError("boom")
        assert _lib._state.recorders == [outer]
    assert _lib._state.recorders == [] and outer.calls == []


def test_driver_side_helpers_of_osmosis_utils(tmp_path):
    """The helpers the reference's sampling scripts call on `osmosis_utils.utils` (osmosis_sampling.py, RGBD_prior_sampling.py):
    `change_input_output_unet` (utils.py:265-288) on this package's UNetModel, `clip_image` (:138-159), `load_yaml` /
    `arguments_from_file` (:357-360, :466-476)."""
    import math
    from osmosis_diffusion_code_amd.guided_diffusion.unet import UNetModel, create_model
    from osmosis_diffusion_code_amd.osmosis_utils import utils as U
    # RGBD_prior_sampling.py:62-69: a 3 -> 6 network, then 4 -> 8
    m = UNetModel(image_size=256, in_channels=3, out_channels=6, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 2),
                  attention_resolutions=[2, 4], num_head_channels=16, dropout=0.1, resblock_updown=True, use_scale_shift_norm=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert before["input_blocks.0.0.weight"].shape == (32, 3, 3, 3) and before["out.2.weight"].shape == (6, 32, 3, 3)
    assert U.change_input_output_unet(m, in_channels=4, out_channels=8) is m
    sd = m.state_dict()
    changed = ("input_blocks.0.0.weight", "input_blocks.0.0.bias", "out.2.weight", "out.2.bias")
    assert sd["input_blocks.0.0.weight"].shape == (32, 4, 3, 3) and sd["out.2.weight"].shape == (8, 32, 3, 3) and sd["out.2.bias"].shape == (8,)
    assert (m.in_channels, m.out_channels) == (4, 8) and list(sd) == list(before)
    assert all(torch.equal(before[k], sd[k]) for k in sd if k not in changed)
    for k, fan_in in (("input_blocks.0.0", 4 * 9), ("out.2", 32 * 9)):           # nn.Conv2d's default initialisation
        bound = 1.0 / math.sqrt(fan_in)
        assert float(sd[k + ".weight"].abs().max()) <= bound and float(sd[k + ".bias"].abs().max()) <= bound
        assert float(sd[k + ".weight"].std()) > 0.3 * bound
    ref = create_model(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
                       num_head_channels=16, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True, pretrain_model="osmosis")
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(ref.state_dict(), strict=True)          # a checkpoint of the 4 -> 8 network loads (RGBD_prior_sampling.py:72)
    # clip_image
    g = torch.Generator().manual_seed(1)
    img = torch.randn(3, 5, 7, generator=g) * 1.5
    keep = img.clone()
    u8 = U.clip_image(img, scale=True, move=True, is_uint8=True)
    assert u8.dtype == torch.uint8 and torch.equal(u8, ((0.5 * (img + 1)) * 255).clamp(0, 255).to(torch.uint8)) and torch.equal(img, keep)
    assert torch.equal(U.clip_image(img, scale=False, move=False, is_uint8=True), (img * 255).clamp(0, 255).to(torch.uint8))
    f = U.clip_image(img[0], scale=True, move=True, is_uint8=False)
    assert f.shape == (1, 5, 7) and float(f.min()) >= 0.0 and float(f.max()) <= 1.0 and torch.equal(img, keep)
    # YAML -> Namespace
    p = tmp_path / "c.yaml"
    p.write_text("manual_seed: 4321\nnumber_of_images: 5\ndiffusion:\n  steps: 1000\n  noise_schedule: linear\nunet_model:\n  model_path: ./m.pt\n  attention_resolutions: 32, 16, 8\n")
    args = U.arguments_from_file(str(p))
    assert args.manual_seed == 4321 and args.number_of_images == 5 and args.diffusion["steps"] == 1000
    assert args.unet_model["attention_resolutions"] == "32, 16, 8" and U.load_yaml(str(p))["unet_model"]["model_path"] == "./m.pt"


def test_get_optimizer_factory():
    """utils.get_optimizer (utils.py:494-524) as a third-party operator would call it: torch.optim classes by case-insensitive name
    with per-group learning rates, None for GD, ValueError for an unknown name."""
    from osmosis_diffusion_code_amd.osmosis_utils import utils as U
    a, b = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
    groups = [{"params": a, "lr": 1e-3}, {"params": b, "lr": 2e-3}]
    for name, cls in (("adam", torch.optim.Adam), ("SGD", torch.optim.SGD), ("RMSprop", torch.optim.RMSprop), ("adagrad", torch.optim.Adagrad),
                      ("adadelta", torch.optim.Adadelta), ("AdamW", torch.optim.AdamW), ("adamax", torch.optim.Adamax),
                      ("asgd", torch.optim.ASGD), ("rprop", torch.optim.Rprop), ("lbfgs", torch.optim.LBFGS)):
        opt = U.get_optimizer(optimizer_name=name, model_parameters=[dict(g) for g in groups] if name != "lbfgs" else [a, b])
        assert type(opt) is cls, name
        if name != "lbfgs":
            assert [g["lr"] for g in opt.param_groups] == [1e-3, 2e-3]
    assert U.get_optimizer("GD", groups) is None and U.get_optimizer("", groups) is None
    with pytest.raises(ValueError, match="not supported"):
        U.get_optimizer("nadam", groups)


def test_bench_dump_outputs_names_dtypes_and_sample(tmp_path):
    """bench.py --dump-outputs: one .npy per output of the timed path (tensors float32, loss float64, ranks > 0 prefixed), and an
    output larger than DUMP_MAX_ELEMS replaced by the same seeded sample of its values on every call."""
    import bench
    n = bench.DUMP_MAX_ELEMS + 1000
    big = torch.arange(n, dtype=torch.float64)
    out = (big, {"phi_a": torch.ones(1, 3), "phi_inf": torch.zeros(1, 3)}, [0.25], torch.ones(1, 4, 8, 8, dtype=torch.float16))
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out, rank=1)
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy", "phi_a.npy", "phi_inf.npy", "pred_xstart.npy", "x_t.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == ["rank1_" + f for f in sorted(os.listdir(tmp_path / "a"))]
    x = np.load(tmp_path / "a" / "x_t.npy")
    assert x.dtype == np.float32 and x.shape == (bench.DUMP_MAX_ELEMS,) and len(np.unique(x)) == x.size
    assert np.array_equal(x, np.load(tmp_path / "b" / "rank1_x_t.npy"))
    x0 = np.load(tmp_path / "a" / "pred_xstart.npy")
    assert x0.dtype == np.float32 and x0.shape == (1, 4, 8, 8) and (x0 == 1).all()
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [0.25]
    bench.dump_outputs(str(tmp_path / "c"), out, rank=3, world=4)        # the cap is shared by the ranks of the job
    assert np.load(tmp_path / "c" / "rank3_x_t.npy").shape == (bench.DUMP_MAX_ELEMS // 4,)
