"""CPU-only checks of the image-folder data set: the new entry points are bound and refuse bad arguments on the host, the command
line picks its image source as documented (`train.dataset_source`), a folder is refused before the GPU is touched when a file does
not fit, and the numpy multi-Otsu reference (tests/multiotsu_ref.py) gives the hand-computed answers."""
import ctypes
import os
import types

import numpy as np
import pytest

import multiotsu_ref as M

NEW_SYMBOLS = ("ngan_u8_histogram", "ngan_multiotsu4_noise_stats", "ngan_u8_pad_noise_fill", "ngan_multiotsu_workspace_bytes")


@pytest.fixture(scope="module")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def test_dataset_entry_points_are_bound_and_validate_on_the_host(built):
    lib = built._C.lib()
    for name in NEW_SYMBOLS:
        assert name in built._C.exported_symbols() and hasattr(lib, name)
    p = ctypes.c_void_p(4096)            # any non-null, 16-byte aligned address: every call below is refused before a launch
    assert lib.ngan_multiotsu_workspace_bytes(3) > 0 and lib.ngan_multiotsu_workspace_bytes(0) == 0
    assert lib.ngan_multiotsu_workspace_bytes(6) == 2 * lib.ngan_multiotsu_workspace_bytes(3)
    cases = [
        ("null", lambda: lib.ngan_u8_histogram(None, p, 1, 64, None)),
        ("null", lambda: lib.ngan_u8_histogram(p, None, 1, 64, None)),
        ("positive", lambda: lib.ngan_u8_histogram(p, p, 0, 64, None)),
        ("positive", lambda: lib.ngan_u8_histogram(p, p, -2, 64, None)),
        ("positive", lambda: lib.ngan_u8_histogram(p, p, 1, 0, None)),
        ("unsupported", lambda: lib.ngan_u8_histogram(p, p, 1, 2 ** 23 + 1, None)),
        ("null", lambda: lib.ngan_multiotsu4_noise_stats(None, p, p, p, p, 1, None)),
        ("null", lambda: lib.ngan_multiotsu4_noise_stats(p, None, p, p, p, 1, None)),
        ("null", lambda: lib.ngan_multiotsu4_noise_stats(p, p, p, p, None, 1, None)),
        ("positive", lambda: lib.ngan_multiotsu4_noise_stats(p, p, p, p, p, 0, None)),
        ("null", lambda: lib.ngan_u8_pad_noise_fill(None, p, p, p, 1, 64, None)),
        ("null", lambda: lib.ngan_u8_pad_noise_fill(p, p, p, None, 1, 64, None)),
        ("positive", lambda: lib.ngan_u8_pad_noise_fill(p, p, p, p, 0, 64, None)),
        ("positive", lambda: lib.ngan_u8_pad_noise_fill(p, p, p, p, 1, 0, None)),
        ("unsupported", lambda: lib.ngan_u8_pad_noise_fill(p, p, p, p, 1, 2897, None)),     # 2897^2 > 2^23
        ("aligned", lambda: lib.ngan_u8_pad_noise_fill(p, p, p, ctypes.c_void_p(4100), 1, 64, None)),
    ]
    for word, call in cases:
        assert call() < 0
        assert word.encode() in lib.ngan_last_error(), (word, lib.ngan_last_error())


def _source(ngan, argv, dataset_dir, default, images=""):
    options = types.SimpleNamespace(images=images)
    config = types.SimpleNamespace(dataset_dir=dataset_dir, configs_name={"dataset_dir": default})
    return ngan.train.dataset_source(argv, options, config)


def test_dataset_source_covers_the_four_cases(ngan, tmp_path):
    folder, missing, default = str(tmp_path), str(tmp_path / "nowhere"), str(tmp_path / "data" / "science_2022")
    # --images wins, whatever dataset_dir is
    assert _source(ngan, ["--images", "x.pt"], missing, default, images="x.pt") == "images"
    assert _source(ngan, ["--images", "x.pt", "--dataset_dir", folder], folder, default, images="x.pt") == "images"
    # an existing folder, named on the command line or by the configuration file
    assert _source(ngan, ["--dataset_dir", folder], folder, default) == "directory"
    assert _source(ngan, ["--configs", "tiny.py"], folder, default) == "directory"
    # the package's default folder, absent in a checkout: synthetic images, as before
    assert _source(ngan, [], default, default) == "synthetic"
    assert _source(ngan, ["--configs", "tiny.py", "--pggan"], default, default) == "synthetic"
    # a folder somebody named that does not exist: the reference's error
    with pytest.raises(ValueError, match="The dataset path .*nowhere does not exist"):
        _source(ngan, ["--dataset_dir", missing], missing, default)
    with pytest.raises(ValueError, match="does not exist"):
        _source(ngan, ["--configs", "tiny.py"], missing, default)          # named in the configuration file
    with pytest.raises(ValueError, match="does not exist"):
        _source(ngan, ["--dataset_dir", default], default, default)         # even the default, once it is named
    # and the real configuration module's default is the one that falls back
    from types import SimpleNamespace
    cfg = ngan.configs.config
    assert not os.path.exists(cfg.configs_name["dataset_dir"])
    assert ngan.train.dataset_source([], SimpleNamespace(images=""), SimpleNamespace(
        dataset_dir=os.path.abspath(cfg.configs_name["dataset_dir"]), configs_name=cfg.configs_name)) == "synthetic"


def test_a_missing_folder_is_the_references_error(ngan, tmp_path):
    missing = str(tmp_path / "nowhere")
    with pytest.raises(ValueError) as e:
        ngan.data.NeuronDataset.from_directory(missing)
    assert str(e.value) == "The dataset path {} does not exist.".format(missing)


def _save(path, array):
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(array).save(path)


def test_a_folder_is_refused_before_the_gpu_is_touched(ngan, tmp_path):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(0)
    grey = lambda h, w: rng.integers(0, 256, (h, w), dtype=np.uint8)
    from_directory = ngan.data.NeuronDataset.from_directory

    rgb = tmp_path / "rgb"
    rgb.mkdir()
    _save(rgb / "a.png", grey(8, 8))
    _save(rgb / "b.png", rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"b\.png.*mode 'RGB'"):
        from_directory(str(rgb))

    wide = tmp_path / "wide"
    wide.mkdir()
    _save(wide / "a.png", grey(8, 12))
    with pytest.raises(ValueError, match=r"a\.png.*12 x 8.*square"):
        from_directory(str(wide))

    sizes = tmp_path / "sizes"
    sizes.mkdir()
    _save(sizes / "a.png", grey(8, 8))
    _save(sizes / "b.png", grey(16, 16))
    with pytest.raises(ValueError, match=r"b\.png.*16 pixels wide, expected 8"):
        from_directory(str(sizes))
    with pytest.raises(ValueError, match=r"a\.png.*8 pixels wide, expected 16 \(image_size\)"):
        from_directory(str(sizes), image_size=16)


def test_hidden_files_are_skipped_and_the_order_is_sorted(ngan, tmp_path):
    pytest.importorskip("PIL")
    images = {name: np.full((8, 8), level, dtype=np.uint8) for name, level in (("c.png", 3), ("a.png", 1), ("b.png", 2))}
    for name, img in images.items():                       # written in an order that is not the sorted one
        _save(tmp_path / name, img)
    (tmp_path / ".DS_Store").write_bytes(b"not an image")
    (tmp_path / "subfolder").mkdir()
    arrays, filenames = ngan.data.read_image_folder(str(tmp_path), image_size=8)
    assert [os.path.basename(f) for f in filenames] == ["a.png", "b.png", "c.png"]
    assert arrays.dtype == np.uint8 and arrays.shape == (3, 8, 8)
    assert [int(a[0, 0]) for a in arrays] == [1, 2, 3]


def test_reference_on_hand_made_histograms():
    # four occupied levels: the only partition into four non-empty classes wins, and its smallest triplet is the first three levels
    h = np.zeros(256, dtype=np.int64)
    h[[3, 9, 40, 200]] = [5, 6, 7, 8]
    triplet, best, second = M.multiotsu4(h)
    assert triplet == (3, 9, 40)
    assert best == 15.0 ** 2 / 5 + 54.0 ** 2 / 6 + 280.0 ** 2 / 7 + 1600.0 ** 2 / 8
    assert second is not None and second < best
    # an empty stretch: every t1 in 12..99 cuts {10, 11, 12} from {100, 101} the same way; the smallest triplet of the tie class
    h = np.zeros(256, dtype=np.int64)
    h[[10, 11, 12, 100, 101, 180, 181, 250]] = [50, 60, 50, 30, 30, 20, 20, 40]
    triplet, best, second = M.multiotsu4(h)
    assert triplet == (12, 101, 181)
    pp, sp = M.prefix_sums(h)
    c = M.class_scores(pp, sp)
    for other in ((12, 101, 181), (50, 150, 200), (99, 179, 249)):          # the same cut, larger triplets: the same bits
        t0, t1, t2 = other
        assert ((c[10, t0] + c[t0 + 1, t1]) + c[t1 + 1, t2]) + c[t2 + 1, 250] == best
    assert M.relative_gap(best, second) > 1e-3
    # fewer than four levels: refused, as skimage does
    h = np.zeros(256, dtype=np.int64)
    h[[0, 7, 9]] = 4
    with pytest.raises(ValueError):
        M.multiotsu4(h)
    # the noise record takes the reference's strict comparisons
    img = np.array([[0, 1, 5], [9, 10, 200]], dtype=np.uint8)
    assert M.noise_record(img, 10) == (3, 5.0, float(np.std([1.0, 5.0, 9.0])))


def test_the_generator_is_seeded_and_micrograph_like():
    a, b = M.micrograph(7, 64), M.micrograph(7, 64)
    assert a.dtype == np.uint8 and a.shape == (64, 64) and np.array_equal(a, b)
    assert not np.array_equal(a, M.micrograph(8, 64))
    assert a[0, 0] == 0 and a[32, 32] != 0 and 0.2 < (a == 0).mean() < 0.5
    triplet, best, second = M.multiotsu4(np.bincount(a.ravel(), minlength=256))
    assert 22 < triplet[0] < 50 < triplet[1] < 110 < triplet[2] < 190
    count, mean, std = M.noise_record(a, triplet[0])
    assert count > 1000 and abs(mean - 18.0) < 0.5 and abs(std - 4.0) < 0.5
