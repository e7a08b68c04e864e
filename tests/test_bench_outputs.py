"""bench.py --dump-outputs without a GPU: dump_outputs() on CPU tensors shaped like the headline step's outputs (16 pairs of 1242x375)."""
import numpy as np
import torch

import bench


def headline_outputs(seed):
    g = torch.Generator().manual_seed(seed)
    B, h, w, cap = 16, 375, 1242, 4096
    ncomp = torch.randint(0, 2 * cap, (B,), dtype=torch.int32, generator=torch.Generator().manual_seed(0))
    # rows past n_components are undefined: different garbage for every seed
    table = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, cap, 7), dtype=torch.int32, generator=torch.Generator().manual_seed(5))
    undefined = torch.arange(cap)[None, :] >= ncomp[:, None]
    table[undefined] = torch.randint(-2 ** 31, 2 ** 31 - 1, (int(undefined.sum()), 7), dtype=torch.int32, generator=g)
    return {"disparity": torch.randint(-16, 2048, (B, h, w), dtype=torch.int16, generator=torch.Generator().manual_seed(1)),
            "planes": torch.randint(0, 4, (B, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)),
            "params": torch.randint(-64, 64, (B, 6), dtype=torch.int32, generator=torch.Generator().manual_seed(3)),
            "ids": torch.randint(0, 2 ** 31 - 1, (B, h, w), dtype=torch.int32, generator=torch.Generator().manual_seed(4)),
            "components": table, "n_components": ncomp, "done": object()}


def test_dump_fits_its_budget_exactly_and_does_not_depend_on_undefined_rows(tmp_path):
    dumps = []
    for seed in (10, 11):
        out = headline_outputs(seed)
        bench.dump_outputs(out, str(tmp_path / str(seed)))
        files = sorted((tmp_path / str(seed)).iterdir())
        assert [f.name for f in files] == sorted(k + ".npy" for k in out if k != "done")
        assert sum(f.stat().st_size for f in files) <= bench.DUMP_BYTES
        dumps.append({f.stem: np.load(f) for f in files})
    a, b = dumps
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["disparity"].dtype == np.float32 and a["planes"].dtype == np.float32
    assert a["ids"].dtype == np.float64 and a["components"].dtype == np.float64
    # small outputs are whole and exact; defined table rows kept, the rest zero
    assert np.array_equal(a["params"], out["params"].numpy()) and np.array_equal(a["n_components"], out["n_components"].numpy())
    t, n = out["components"].numpy(), np.minimum(out["n_components"].numpy(), 4096)
    for f in range(16):
        assert np.array_equal(a["components"][f, :n[f]], t[f, :n[f]]) and not a["components"][f, n[f]:].any()
    # the per-pixel outputs do not fit whole: exact values at the documented sample indices
    for k in ("disparity", "planes", "ids"):
        full = out[k].numpy().reshape(-1)
        got = a[k]
        assert got.ndim == 1 and 0.25 * full.size < got.size < full.size, k
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(full.size, got.size, replace=False))
        assert np.array_equal(got, full[idx].astype(got.dtype)) and np.array_equal(got.astype(np.int64), full[idx]), k


def test_small_outputs_are_written_whole(tmp_path):
    out = {"disparity": (torch.arange(4 * 96 * 320) % 2048).to(torch.int16).reshape(4, 96, 320), "done": None}
    bench.dump_outputs(out, str(tmp_path))
    d = np.load(tmp_path / "disparity.npy")
    assert d.dtype == np.float32 and d.shape == (4, 96, 320) and np.array_equal(d, out["disparity"].numpy())
