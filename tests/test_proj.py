"""Visual-feature injection: depth rendering (proj2img) and back-projection (I2P).
CPU: the oracle restatement against vectors recorded from the reference (tests/golden/make_fixtures_proj.py).
GPU: the HIP kernels against the same vectors and against the oracle at the real sizes.
These are whole-image / whole-tensor checks on benign clouds; the per-pixel and per-element checks on planted inputs (border shift,
collisions, cancellation, lattice quotients, every tap class of the back-projection, the out= / col form) live in
tests/test_gpu_visual_elements.py, with tests/visual_ref.py and tests/test_visual_ref_cpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref

CASES = ["small", "dense", "up"]


def _backbone(g):
    w, b, stride = torch.from_numpy(g["conv_w"]), torch.from_numpy(g["conv_b"]), int(g["stride"])
    return lambda img: torch.tanh(F.conv2d(img, w.to(img.device), b.to(img.device), stride=stride, padding=2))


def _view1(x):
    c, s = np.cos(-np.pi / 2), np.sin(-np.pi / 2)
    rot = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64).float()
    return torch.bmm(x.permute(0, 2, 1), rot[None].repeat(x.shape[0], 1, 1))


def _codes(img):
    """(B,3,224,224) colours -> colour-table index per pixel, 256 for the -1 background."""
    lut = torch_ref.piyg_lut().to(img.device)
    flat = img.permute(0, 2, 3, 1).reshape(-1, 3)
    code = torch.full((flat.shape[0],), 256, dtype=torch.int64, device=img.device)
    live = flat[:, 0] != -1
    d = (flat[live][:, None, :] - lut[None]).abs().sum(-1)
    assert float(d.min(1)[0].max()) == 0.0                        # every colour IS a table entry
    code[live] = d.argmin(1)
    return code.view(img.shape[0], 224, 224).cpu().numpy()


def _check_image(code, want):
    want = want.astype(np.int64)
    assert np.array_equal(code == 256, want == 256)               # the empty-pixel mask is exact
    diff = np.abs(code - want)
    # summation order of the depths differs (sequential fp32 in the reference): a pixel may land in the next table bin
    assert diff.max() <= 1 and (diff > 0).mean() < 2e-3, (diff.max(), (diff > 0).mean())


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference(golden, case):
    g = golden("proj_" + case)
    x = torch.from_numpy(g["x"])
    pts = _view1(x)
    img, pc_min, grid, offs = torch_ref.proj2img(pts)
    _check_image(_codes(img), g["img_code"])
    assert np.array_equal(pc_min.numpy(), g["pc_min"]) and np.array_equal(grid.numpy(), g["grid_size"])
    assert np.array_equal(offs[0].numpy(), g["offset_x"]) and np.array_equal(offs[1].numpy(), g["offset_y"])
    feats = _backbone(g)(img)
    assert tuple(feats.shape[2:]) == tuple(g["feat_hw"])
    np.testing.assert_allclose(torch_ref.i2p(pts, feats, pc_min, grid, offs).numpy(), g["i2p_view1"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(torch_ref.visual_features(x, _backbone(g)).numpy(), g["clip_feats"], rtol=0, atol=2e-5)


def test_piyg_table_endpoints():
    lut = torch_ref.piyg_lut()
    assert lut.shape == (256, 3)
    np.testing.assert_allclose(lut[0].numpy(), np.array([142, 1, 82]) / 255.0, atol=1e-7)
    np.testing.assert_allclose(lut[255].numpy(), np.array([39, 100, 25]) / 255.0, atol=1e-7)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_hip_matches_reference(golden, case):
    from dvm import ops
    from models.model import Uni3FC, rotate_point_cloud_batch_torch
    g = golden("proj_" + case)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(g["x"]).to(dev)
    pts = rotate_point_cloud_batch_torch(x, -np.pi / 2, axis='z')
    np.testing.assert_allclose(pts.cpu().numpy(), _view1(torch.from_numpy(g["x"])).numpy(), rtol=0, atol=1e-7)
    net = Uni3FC(k=8)
    img, pc_min, grid, offs = net.proj2img(pts)
    assert img.shape == (x.shape[0], 3, 224, 224) and pc_min.shape == (x.shape[0], 1, 2) and grid.shape == (x.shape[0], 1, 1)
    _check_image(_codes(img), g["img_code"])
    assert np.array_equal(pc_min.cpu().numpy(), g["pc_min"]) and np.array_equal(grid.cpu().numpy(), g["grid_size"])
    assert np.array_equal(offs[0].cpu().numpy(), g["offset_x"]) and np.array_equal(offs[1].cpu().numpy(), g["offset_y"])
    img2 = net.proj2img(pts)[0]
    assert torch.equal(img, img2)                                   # fixed-point depth sums: bit-reproducible
    # back-projection on the reference's own image/features, so that a flipped pixel above cannot leak into this check
    ref_img = torch_ref.proj2img(_view1(torch.from_numpy(g["x"])))[0]
    feats = _backbone(g)(ref_img).to(dev)
    got = net.I2P(pts, feats, pc_min, grid, offs)
    np.testing.assert_allclose(got.cpu().numpy(), g["i2p_view1"], rtol=0, atol=2e-5)
    # the whole branch through Uni3FC.forward's entry (dino_feat=None)
    clip = net.visual_features(x, _backbone(g))
    err = np.abs(clip.cpu().numpy() - g["clip_feats"]).max(-1)
    assert np.median(err) < 1e-5 and (err > 1e-4).mean() < 0.02, (np.median(err), err.max(), (err > 1e-4).mean())


@pytest.mark.gpu
def test_hip_full_size_against_oracle():
    """The shipped shape: N = 4995 points, 384-channel 256x256 feature maps (DINOv2 ViT-S/14 through FeatUp)."""
    from dvm import ops
    from models.model import Uni3FC_DINO_proj
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 4995, generator=g) * torch.tensor([0.2, 0.5, 0.15]).view(1, 3, 1)
    pts = _view1(x)
    img_o, pc_min_o, grid_o, offs_o = torch_ref.proj2img(pts)
    img, pc_min, grid, off = ops.proj2img(pts.to(dev))
    _check_image(_codes(img), _codes(img_o))
    assert torch.equal(pc_min.cpu().view(1, 1, 2), pc_min_o) and torch.equal(grid.cpu().view(1, 1, 1), grid_o)
    f = torch.randn(1, 384, 256, 256, generator=g)
    want = F.normalize(torch_ref.i2p(pts, f, pc_min_o, grid_o, offs_o), dim=-1)
    got = ops.i2p(pts.to(dev), f.to(dev), pc_min, grid, off, normalize=True)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=0, atol=1e-5)
    # module level: three views into one (B,N,1152) tensor
    up = lambda im: torch.tanh(F.conv2d(im, torch.ones(384, 3, 1, 1, device=im.device) * 0.1))   # noqa: E731
    out = Uni3FC_DINO_proj()(x.to(dev), up)
    assert out.shape == (1, 4995, 1152)
    np.testing.assert_allclose(out.norm(dim=-1).cpu().numpy(), np.sqrt(3.0), rtol=1e-5)


@pytest.mark.gpu
def test_forward_without_precomputed_features():
    """Uni3FC.forward(x, None, upsampler) == Uni3FC.forward(x, visual_features(x, upsampler), None)."""
    from models.model import Uni3FC
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = Uni3FC(k=16).to(dev).eval()
    x = torch.rand(2, 3, 300, device=dev)
    w = torch.randn(384, 3, 3, 3, device=dev) * 0.3
    up = lambda im: F.conv2d(im, w, stride=2, padding=1)                                          # noqa: E731
    with torch.no_grad():
        a = net(x, None, up)[0]
        b = net(x, net.visual_features(x, up), None)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        net(x, None, None)
