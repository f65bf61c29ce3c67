"""The fused SSIM loss without a GPU: the float64 spec (tests/ssim_spec.py) against torch autograd of the reference's
formula, the C ABI's size checks and workspace query, hgs.loss.ssim's argument checks, and the kernels' resources."""
import ctypes as C
import os
import shutil
import sys

import pytest
import torch

import ssim_spec
import train_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")


def _image(kind, C_, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(C_, H, W, generator=g, dtype=torch.float64)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64),
                            indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(3 * xx + 2 * yy + k) for k in range(C_)])
    if kind == "smooth":
        return base
    assert kind == "flat"
    img = base + 0.05 * torch.rand(C_, H, W, generator=g, dtype=torch.float64)
    img[:, H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 0.3
    return img


CASES = [("random", 3, 23, 31), ("smooth", 3, 40, 52), ("flat", 3, 37, 53), ("random", 1, 16, 16),
         ("smooth", 4, 21, 19), ("random", 3, 7, 30), ("flat", 1, 30, 5), ("random", 3, 8, 9), ("random", 4, 1, 1),
         ("smooth", 3, 33, 65)]


@pytest.mark.parametrize("kind,C_,H,W", CASES)
def test_spec_matches_autograd_of_the_reference_formula(kind, C_, H, W):
    x1 = _image(kind, C_, H, W, 1)
    x2 = (0.7 * x1 + 0.3 * _image("random", C_, H, W, 2)).clamp(0, 1)
    if kind == "flat":
        x2[:, H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 0.3          # a region that is flat in both images
    a = x1.clone().requires_grad_(True)
    ref = train_loop.ssim(a, x2)
    ref.backward()
    val, grad = ssim_spec.ssim_and_grad(x1, x2)
    assert abs(val.item() - ref.item()) <= 1e-12 * abs(ref.item())
    assert (grad - a.grad).abs().max().item() <= 1e-12 * a.grad.abs().max().item()


def test_spec_per_image_mean_and_upstream_vector():
    x1 = torch.rand(2, 3, 20, 24, dtype=torch.float64)
    x2 = torch.rand(2, 3, 20, 24, dtype=torch.float64)
    g = torch.tensor([0.7, -1.3], dtype=torch.float64)
    a = x1.clone().requires_grad_(True)
    ref = torch.stack([train_loop.ssim(a[i], x2[i]) for i in range(2)])
    (ref * g).sum().backward()
    val, grad = ssim_spec.ssim_and_grad(x1, x2, size_average=False, grad_out=g)
    assert val.shape == (2,)
    assert torch.allclose(val, ref.detach(), rtol=1e-12, atol=0)
    assert (grad - a.grad).abs().max().item() <= 1e-12 * a.grad.abs().max().item()


# -- C ABI: no GPU needed -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from hgs import _lib
    return _lib.lib()


def test_tmp_bytes_query_needs_no_gpu(lib):
    # one double per 32x16 tile of every (image, channel) plane, 256-byte aligned
    n = lib.hgs_ssim_tmp_bytes(1, 3, 1080, 1920)
    assert n >= 3 * 60 * 68 * 8 and n % 256 == 0
    assert lib.hgs_ssim_tmp_bytes(8, 3, 1080, 1920) >= 8 * 3 * 60 * 68 * 8
    assert lib.hgs_ssim_tmp_bytes(1, 1, 1, 1) >= 8


@pytest.mark.parametrize("dims", [(0, 3, 10, 10), (1, 0, 10, 10), (1, 3, 0, 10), (1, 3, 10, -1), (-2, 3, 10, 10),
                                  (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 20, 1, 64)])
def test_bad_sizes_are_refused_before_any_hip_call(lib, dims):
    assert lib.hgs_ssim_tmp_bytes(*dims) == 0
    assert b"bad sizes" in lib.hgs_last_error()
    p = C.c_void_p(16)      # never dereferenced: the size check comes first
    assert lib.hgs_ssim_fwd(p, p, *dims, p, p, p, p, None, 0) != 0
    assert b"bad sizes" in lib.hgs_last_error()
    assert lib.hgs_ssim_bwd(p, p, p, p, 0, *dims, p, None, 0) != 0
    assert b"bad sizes" in lib.hgs_last_error()


def test_tile_count_limit_of_a_one_dimensional_grid(lib):
    """One 256-thread workgroup per 32x16 tile in a 1-D grid whose work-item count is 32 bits: at most
    (2^32 - 1) // 256 = 16 777 215 tiles.  65536x131072 is 4096 x 4096 = 2^24 tiles, one too many; 65536x131040 is
    4096 x 4095 tiles, inside the limit."""
    limit = (2 ** 32 - 1) // 256
    over, under = (1, 1, 65536, 131072), (1, 1, 65536, 131040)
    tiles = lambda d: d[0] * d[1] * -(-d[2] // 16) * -(-d[3] // 32)
    assert tiles(over) == limit + 1 and tiles(under) <= limit
    assert lib.hgs_ssim_tmp_bytes(*over) == 0
    assert b"16777215 tiles" in lib.hgs_last_error() and b"2^32 - 1 work-items" in lib.hgs_last_error()
    p = C.c_void_p(16)      # never dereferenced: the size check comes first
    assert lib.hgs_ssim_fwd(p, p, *over, p, p, p, p, None, 0) != 0
    assert b"16777215 tiles" in lib.hgs_last_error()
    assert lib.hgs_ssim_bwd(p, p, p, p, 1, *over, p, None, 0) != 0
    assert b"16777215 tiles" in lib.hgs_last_error()
    n = lib.hgs_ssim_tmp_bytes(*under)
    assert n >= tiles(under) * 8 and n % 256 == 0
    # the limit counts the tiles of every (image, channel) plane
    assert lib.hgs_ssim_tmp_bytes(3, 1, 65536, 131040) == 0 and lib.hgs_ssim_tmp_bytes(1, 3, 65536, 131040) == 0
    assert lib.hgs_ssim_tmp_bytes(limit, 1, 16, 32) > 0 and lib.hgs_ssim_tmp_bytes(limit + 1, 1, 16, 32) == 0


def test_null_pointers_are_refused(lib):
    p = C.c_void_p(256)
    assert lib.hgs_ssim_fwd(None, p, 1, 3, 8, 8, p, p, None, p, None, 0) != 0
    assert b"null argument" in lib.hgs_last_error()
    assert lib.hgs_ssim_bwd(p, p, None, p, 0, 1, 3, 8, 8, p, None, 0) != 0
    assert b"null argument" in lib.hgs_last_error()


# -- hgs.loss.ssim: argument checks (they come before any device work) -------------------------------------------------

def test_ssim_rejects_bad_arguments_and_cpu_tensors():
    from hgs import loss
    a, b = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    with pytest.raises(ValueError, match="window_size"):
        loss.ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="shapes differ"):
        loss.ssim(a, b[:, :8])
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(N,C,H,W\)"):
        loss.ssim(a[0], b[0])
    with pytest.raises(ValueError, match="size_average=False"):
        loss.ssim(a, b, size_average=False)
    with pytest.raises(ValueError, match="only img1"):
        loss.ssim(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="float32"):
        loss.ssim(a.double(), b.double())
    with pytest.raises(ValueError, match="float32"):
        loss.ssim(a.half(), b.half())
    with pytest.raises(ValueError, match="GPU tensor"):
        loss.ssim(a, b)
    with pytest.raises(ValueError, match="GPU tensor"):
        loss.ssim(a[None], b[None], size_average=False)


def test_l1_loss_is_the_reference_expression():
    from hgs import loss
    a, b = torch.rand(3, 5, 7), torch.rand(3, 5, 7)
    assert torch.equal(loss.l1_loss(a, b), torch.abs(a - b).mean())


# -- kernel resources ---------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_ssim_kernels_compile_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources.collect([os.path.join(CSRC, "ssim.hip")])}
    assert {"ssim_fwd_kernel", "ssim_bwd_kernel", "ssim_reduce_kernel"} <= set(rows)
    for name, r in rows.items():
        assert r["scratch"] == 0 and r["spills"] == 0, (name, r)
    for name in ("ssim_fwd_kernel", "ssim_bwd_kernel"):          # memory-bound: keep at least 6 waves per SIMD
        assert min(rows[name]["waves_regs"], rows[name]["waves_lds"]) >= 6, rows[name]
