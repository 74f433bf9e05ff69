"""Device-resident data set, the parts that need no GPU: the numpy restatement of the contract (tests/data_reference.py) against the
published known answers, the step -> (epoch, first) arithmetic, the rank tiling, the train.py flag and the ABI exports."""
import numpy as np
import pytest

import data_reference as R


def words(c, k):
    return [int(w) for w in R.philox(*c, *k)]


def test_philox_known_answers():
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert words((f, f, f, f), (f, f)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_key_is_the_two_halves_of_the_seed():
    assert R.key(0x299F31D0A4093822) == (0xA4093822, 0x299F31D0)


def test_uniforms_are_exact_and_open():
    u = R.uniforms(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint64))
    assert u.tolist() == [2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25, 1 - 2.0 ** -25]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 255, 256, 257, 1000, 4097])
def test_restated_permutation_is_a_bijection(N):
    for epoch in (0, 7):
        p = R.perm(3, epoch, N, np.arange(N))
        assert sorted(p.tolist()) == list(range(N))
    if N > 5:
        assert (R.perm(3, 0, N, np.arange(N)) != R.perm(3, 7, N, np.arange(N))).any()
        assert (R.perm(3, 0, N, np.arange(N)) != R.perm(4, 0, N, np.arange(N))).any()


def test_feistel_width():
    assert [R.feistel_bits(N) for N in (1, 2, 3, 4, 5, 16, 17, 256, 257, 65536, 65537, 2 ** 32 - 1)] == [2, 2, 2, 2, 4, 4, 6, 8, 10, 16, 18, 32]


def test_position_arithmetic():
    from mapdit_amd import data
    # N = 100, B = 16: six whole batches per epoch, the last four positions of every epoch are dropped
    assert [data.position(s, 16, 100) for s in (0, 1, 5, 6, 7, 13)] == [(0, 0), (0, 16), (0, 80), (1, 0), (1, 16), (2, 16)]
    assert max(first + 16 for _, first in (data.position(s, 16, 100) for s in range(12))) == 96
    assert data.position(3, 50, 100) == (1, 50)                                  # N % B == 0: nothing dropped
    for s in range(40):
        assert data.position(s, 16, 100) == R.position(s, 16, 100)
    with pytest.raises(ValueError):
        data.position(0, 101, 100)
    with pytest.raises(ValueError):
        data.position(-1, 16, 100)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_rank_shards_tile_the_window(world):
    from mapdit_amd import parallel
    cuts = [parallel.shard_batch(16, r, world) for r in range(world)]
    assert cuts[0][0] == 0 and cuts[-1][1] == 16
    assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))


def test_train_parser_knows_the_flag():
    from mapdit_amd import train
    p = train.build_parser()
    assert p.parse_args(["--results-dir", "r"]).data_loader == "host"
    assert p.parse_args(["--results-dir", "r", "--data-loader", "device"]).data_loader == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--results-dir", "r", "--data-loader", "other"])


def test_synthetic_with_the_device_loader_is_refused_before_any_device_work(tmp_path, monkeypatch):
    import torch
    from mapdit_amd import parallel, train

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(parallel, "init_from_env", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(ValueError, match="--synthetic"):
        train.main(["--synthetic", "--data-loader", "device", "--results-dir", str(tmp_path)])
    assert not list(tmp_path.iterdir())


def test_cpu_device_is_refused():
    import torch
    from mapdit_amd.data import DeviceLatentDataset
    src = (torch.zeros(4, 1, 2, 2), torch.ones(4, 1, 2, 2), torch.zeros(4, dtype=torch.int64), {"mean": [0.0], "std": [1.0]})
    with pytest.raises(NotImplementedError):
        DeviceLatentDataset(src, "cpu")


def test_abi_exports_are_present():
    import ctypes
    from mapdit_amd import _lib as L
    L.build()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name in ("mapdit_philox_normal", "mapdit_data_perm", "mapdit_data_batch"):
        assert name in L.EXPORTS and hasattr(cdll, name), name
    assert cdll.mapdit_abi_version() == 5
