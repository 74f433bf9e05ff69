"""The GEMM K loops stage interior tiles from a scalar base and lane offsets (gemm.hip, "staging of interior tiles"); edge tiles and K
tails keep the per-piece 64-bit lane addresses.  Kernel-level calls through the C ABI on the shapes at which each path can go wrong.

Operands are small integers, so every product and every fp32 partial sum is exact and the result does not depend on the accumulation
order: the comparison with torch in fp64 is ==.  Operands of a 16-bit store are in {-1, 0, 1} (|sum| <= K <= 256: exact in bf16 and
fp16), those of an fp32 store in [-2, 2].  Row strides are larger than the logical widths, the padding holds a value no operand has:
a wrong ld factor in a lane offset or in the K advance, or a read past a row, changes the sums."""
import ctypes as C

import pytest
import torch

DEV = "cuda"
NT, NN, TN = 0, 1, 2
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import mapdit_amd
    return mapdit_amd._lib


@pytest.fixture(params=["bf16", "f16"])
def dt(request):
    return torch.bfloat16 if request.param == "bf16" else torch.float16


@pytest.fixture
def tile256(L):
    """Force the 256^2 kernels for shapes the tile rule would give to the 128^2 kernel (benchmarking hook of the library)."""
    L.lib().gemm_tuning(256, 2, 0)
    yield
    L.lib().gemm_tuning(0, 2, 0)


def ints(rows, cols, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (rows, cols), generator=g).double()


def padded(x, ld, dt):
    """x in the first columns of a [rows, ld] buffer of the operand type; the padding is 7 everywhere."""
    buf = torch.full((x.shape[0], ld), 7.0, dtype=dt, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV).to(dt)
    return buf


def operands(layout, M, N, K, lo, hi, dt, pad_k=64, pad_mn=128, seed=0):
    """(A, B in fp64 as [M, K] and [N, K], device buffers in the layout's storage, lda, ldb)"""
    A, B = ints(M, K, lo, hi, seed + 1), ints(N, K, lo, hi, seed + 2)
    if layout == NT:
        a, b = padded(A, K + pad_k, dt), padded(B, K + pad_k, dt)
    elif layout == NN:
        a, b = padded(A, K + pad_k, dt), padded(B.t(), N + pad_mn, dt)
    else:
        a, b = padded(A.t(), M + pad_mn, dt), padded(B.t(), N + pad_mn, dt)
    return A, B, a, b, a.shape[1], b.shape[1]


def gemm(L, dt, layout, M, N, K, a, lda, b, ldb, out, store_f32, split_k=1):
    ep = L.Epilogue()
    ep.kind = L.EPI_STORE_F32 if store_f32 else L.EPI_STORE_BF16
    ep.out, ep.ldo, ep.alpha = out.data_ptr(), N, 1.0
    if split_k > 1:
        ep.split_k, ep.slab_stride = split_k, M * N
    fn = L.lib().gemm_bf16 if dt == torch.bfloat16 else L.lib().gemm_f16
    fn(layout, M, N, K, a.data_ptr(), lda, b.data_ptr(), ldb, C.byref(ep), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def check(L, dt, layout, M, N, K, store_f32, tile):
    lo, hi = (-2, 2) if store_f32 else (-1, 1)
    A, B, a, b, lda, ldb = operands(layout, M, N, K, lo, hi, dt, seed=layout * 10 + K)
    out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if store_f32 else dt)
    gemm(L, dt, layout, M, N, K, a, lda, b, ldb, out, store_f32)
    assert torch.equal(out.double().cpu(), A @ B.t()), (layout, M, N, K)
    return L.lib().gemm_dma_fast(layout, M, N, K, lda, ldb, tile)


@gpu
@pytest.mark.parametrize("store_f32", [True, False], ids=["shared_image_f32", "wave_private_16bit"])
@pytest.mark.parametrize("K", [192, 128])
@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_interior_tiles_of_the_256_kernels(L, dt, tile256, layout, K, store_f32):
    """2 x 2 tiles of 256^2.  K = 192: prologue, one steady-state K-tile (both DMA groups issued) and the drain; K = 128: the second
    group (K-tile t + 2) is never issued.  fp32 store = the shared-image kernel, 16-bit store = the wave-private one."""
    assert check(L, dt, layout, 512, 512, K, store_f32, 256) == 1


@gpu
def test_persistent_launch_crossing_tiles(L, dt):
    """768 tiles on the wave-private kernel with a plain 16-bit store: three tiles per workgroup, so the next tile's prologue is issued
    from a fresh context while the previous epilogue's stores drain."""
    M, N, K = 256 * 96, 2048, 128
    assert L.lib().gemm_tile_size_k(M, N, K, 0) == 256
    A, B, a, b, lda, ldb = operands(NT, M, N, K, -1, 1, dt, seed=5)
    out = torch.full((M, N), float("nan"), device=DEV, dtype=dt)
    gemm(L, dt, NT, M, N, K, a, lda, b, ldb, out, False)
    assert L.lib().gemm_dma_fast(NT, M, N, K, lda, ldb, 256) == 1
    ref = (A.to(DEV) @ B.to(DEV).t())
    assert torch.equal(out.double(), ref)


@gpu
@pytest.mark.parametrize("forced", [True, False], ids=["256", "128"])
def test_split_k_with_uneven_slabs_tn(L, dt, forced):
    """13 K-tiles over 4 slabs (4, 3, 3, 3): every slab's first K row must reach the scalar base.  Each slab == the product over its own
    K range."""
    M = N = 512
    K, S = 64 * 13, 4
    L.lib().gemm_tuning(256 if forced else 0, 2, 0)
    try:
        assert L.lib().gemm_tile_size_k(M, N, K, 1) == (256 if forced else 128)
        A, B, a, b, lda, ldb = operands(TN, M, N, K, -2, 2, dt, seed=9)
        slabs = torch.full((S, M, N), float("nan"), device=DEV)
        gemm(L, dt, TN, M, N, K, a, lda, b, ldb, slabs, True, split_k=S)
    finally:
        L.lib().gemm_tuning(0, 2, 0)
    assert L.lib().gemm_dma_fast(TN, M, N, K, lda, ldb, 256 if forced else 128) == 1
    k0 = 0
    for z, tiles in enumerate([4, 3, 3, 3]):
        k1 = k0 + 64 * tiles
        assert torch.equal(slabs[z].double().cpu(), A[:, k0:k1] @ B[:, k0:k1].t()), z
        k0 = k1


@gpu
@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_edge_tiles_and_k_tail_keep_the_old_addresses(L, dt, tile256, layout):
    """Clamped rows and columns (M = 520, N = 264) and a K tail (K = 72, zero-sourced pieces) are not interior: the launch must say so and
    the result must be right; the interior shape next to it takes the scalar-base form."""
    assert check(L, dt, layout, 520, 264, 72, True, 256) == 0
    assert check(L, dt, layout, 520, 264, 64, True, 256) == 0
    assert check(L, dt, layout, 512, 256, 72, True, 256) == 0
    assert check(L, dt, layout, 512, 256, 64, True, 256) == 1


@gpu
@pytest.mark.parametrize("store_f32", [True, False], ids=["f32", "16bit"])
@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_the_128_and_64_row_kernels(L, dt, layout, store_f32):
    """[256, 128] over three K-tiles: the 128^2 kernel (fp32 store, and TN), the 64-row kernel (16-bit store, A row-major)."""
    assert L.lib().gemm_tile_size_k(256, 128, 192, 0) == 128
    tile = 64 if (not store_f32 and layout != TN) else 128
    assert check(L, dt, layout, 256, 128, 192, store_f32, tile) == 1
    assert check(L, dt, layout, 264, 136, 192, store_f32, tile) == 0          # ragged: stage_tile


@gpu
def test_grouped_tn_launch_equals_single_launches(L, dt):
    """Two items of different shape in one launch of the group kernel == one launch each, bit for bit, == the product."""
    K = 256
    shapes = [(512, 256), (256, 512)]
    group = L.lib().gemm_group_tn_bf16 if dt == torch.bfloat16 else L.lib().gemm_group_tn_f16
    ops = [operands(TN, r, c, K, -2, 2, dt, seed=30 + i) for i, (r, c) in enumerate(shapes)]
    single = [torch.full((r, c), float("nan"), device=DEV) for r, c in shapes]
    grouped = [torch.full((r, c), float("nan"), device=DEV) for r, c in shapes]
    L.lib().gemm_tuning(256, 2, 0)
    try:
        for (r, c), (A, B, a, b, lda, ldb), o in zip(shapes, ops, single):
            gemm(L, dt, TN, r, c, K, a, lda, b, ldb, o, True)
            assert L.lib().gemm_dma_fast(TN, r, c, K, lda, ldb, 256) == 1
    finally:
        L.lib().gemm_tuning(0, 2, 0)
    items = (L.GemmGroupItem * 2)()
    for i, ((r, c), (A, B, a, b, lda, ldb), o) in enumerate(zip(shapes, ops, grouped)):
        items[i] = L.GemmGroupItem(A=a.data_ptr(), lda=lda, B=b.data_ptr(), ldb=ldb, M=r, N=c, out=o.data_ptr(), ldo=c, alpha=1.0, slab_stride=r * c)
    group(2, C.cast(items, C.c_void_p), K, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (A, B, *_), s, g in zip(ops, single, grouped):
        assert torch.equal(s, g)
        assert torch.equal(g.double().cpu(), A @ B.t())


def test_32_bit_extent_rule():
    """Host logic, nothing allocated: an operand whose rows x ld x 2 bytes fit an unsigned 32-bit offset stages from the scalar base, one
    byte more does not; DiT-B/2's largest operands (256 samples: [65536, 3072] activations) do."""
    import mapdit_amd
    lib = mapdit_amd._lib.lib()
    ok, fast = lib.gemm_dma_extent_ok, lib.gemm_dma_fast
    assert ok((2**32 - 16) // 16, 8) == 1                     # rows * ld * 2 = 2^32 - 16
    assert ok(2**32 // 16, 8) == 0                            # 2^32
    assert ok(65536, 3072) == 1 and ok(65536, 768) == 1 and ok(3072, 768) == 1
    assert ok(0, 8) == 0 and ok(8, 0) == 0
    # fc2 forward / its dX / the fc1 weight gradient at 256 samples
    assert fast(NT, 65536, 768, 3072, 3072, 3072, 256) == 1
    assert fast(NN, 65536, 3072, 768, 768, 3072, 256) == 1
    assert fast(TN, 3072, 768, 65536, 3072, 768, 256) == 1
    # the same launches over a row stride that takes the A operand to 2^32 bytes and beyond
    assert fast(NT, 65536, 768, 3072, 32768, 3072, 256) == 0
    assert fast(NT, 65536, 768, 3072, 32760, 3072, 256) == 1
    assert fast(TN, 3072, 768, 65536, 32768, 768, 256) == 0
    # edges, K tails, unknown tile edges
    assert fast(NT, 520, 264, 64, 64, 64, 256) == 0 and fast(NT, 512, 256, 72, 72, 72, 256) == 0
    assert fast(NT, 512, 256, 64, 64, 64, 256) == 1 and fast(NT, 512, 384, 64, 64, 64, 256) == 0
    assert fast(NT, 512, 384, 64, 64, 64, 128) == 1 and fast(NT, 320, 384, 64, 64, 64, 128) == 0 and fast(NT, 320, 384, 64, 64, 64, 64) == 1
    assert fast(NT, 512, 256, 64, 64, 64, 32) == 0 and fast(3, 512, 256, 64, 64, 64, 256) == 0
