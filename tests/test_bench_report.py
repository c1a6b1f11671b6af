"""bench.py's reporting helpers (CPU): utilisation counters are attached
only from a profiled run of the same workload, and everything they report
(counts and time) comes from that one run."""
import importlib.util
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_util_counters_require_matching_workload(tmp_path, monkeypatch):
    b = _bench()
    cfg = {"width": 3840, "height": 2160, "frames_per_gpu": 256, "quality": 50, "mode": "encode",
           "pipeline": "fused"}
    d = tmp_path / "profiles" / "r99"
    d.mkdir(parents=True)
    k = {"void mij::k_mcu_dct<2>(mij::K1Args)": {"launch_us": 1000.0, "SQ_INSTS_MFMA": 1000000,
                                                 "mfma_util": 0.1, "valu_util": 0.4}}
    (d / "util.json").write_text(json.dumps({"config": cfg, "kernels": k}))
    monkeypatch.setattr(b, "REPO", str(tmp_path))
    u, src = b.util_counters("k_mcu_dct<2>", dict(cfg))
    assert u is not None and src.endswith("util.json")
    f = b.util_fields(u, src)
    # 1e6 MFMA x 32768 ops in the profiled run's own 1 ms
    assert f["mfma_i8_TOPs"] == round(1e6 * 32768 / 1e-3 / 1e12, 1)
    for key, val in (("quality", 90), ("frames_per_gpu", 64), ("pipeline", "split"), ("width", 1920)):
        other = dict(cfg, **{key: val})
        assert b.util_counters("k_mcu_dct<2>", other) == (None, None), key
    # a util.json without a recorded workload is never attached
    (d / "util.json").write_text(json.dumps({"kernels": k}))
    assert b.util_counters("k_mcu_dct<2>", dict(cfg)) == (None, None)


def test_dump_jfif_is_float_deterministic_and_capped(tmp_path, monkeypatch):
    """--dump-outputs: every stream's length and checksums, and whole streams
    of a seeded sample as float32 under the cap; the same streams give the
    same files."""
    import numpy as np
    b = _bench()
    rng = np.random.default_rng(5)
    streams = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()
               for n in rng.integers(1, 4000, size=12)]
    monkeypatch.setattr(b, "DUMP_SAMPLE_VALUES", 6000)
    for d in ("a", "b"):
        b.dump_jfif(str(tmp_path / d), len(streams), lambda i: streams[i])
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["jfif_bytes", "jfif_len", "jfif_sample", "jfif_sum"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["jfif_len"].tolist() == [len(s) for s in streams]
    assert got["jfif_sum"][:, 0].tolist() == [sum(s) for s in streams]
    assert got["jfif_sum"][3, 1] == sum((p + 1) * v for p, v in enumerate(streams[3]))
    keep = [int(i) for i in got["jfif_sample"]]
    assert keep and len(set(keep)) == len(keep)
    assert got["jfif_bytes"].size <= 6000
    assert got["jfif_bytes"].astype(np.uint8).tobytes() == b"".join(streams[i] for i in keep)
    for name, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{name}.npy")), name
    # a first stream longer than the cap is cut to it, not dropped
    monkeypatch.setattr(b, "DUMP_SAMPLE_VALUES", 10)
    b.dump_jfif(str(tmp_path / "c"), len(streams), lambda i: streams[i])
    assert np.load(tmp_path / "c" / "jfif_bytes.npy").size == min(10, len(streams[int(np.load(
        tmp_path / "c" / "jfif_sample.npy")[0])]))


def test_committed_profiles_attach_to_the_default_bench():
    """The newest committed util.json and traffic.json record the workload
    they were measured on, and it is the default bench's (config 3), so the
    driver's bench line carries mfma_util / valu_util and PMC traffic."""
    b = _bench()
    cfg = {"width": 3840, "height": 2160, "frames_per_gpu": 256, "quality": 50, "mode": "encode",
           "pipeline": "fused"}
    u, src = b.util_counters("k_mcu_dct<2>", dict(cfg))
    assert u is not None, "no committed util.json matches the default workload"
    assert 0 < u["mfma_util"] < 1 and 0 < u["valu_util"] < 1
    assert b.pmc_traffic("k_mcu_dct<2>", dict(cfg))[0] is not None
