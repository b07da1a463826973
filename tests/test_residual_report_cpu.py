"""Host side of the residual report (include/lifcal_ba.h section 7j): the exported symbols, the 64-byte row in ctypes and numpy, the
stable counting sort behind the grouped sums (lifcal_group_index) and the CSV writer of a table (lifcal_write_group_stats_csv)."""
import ctypes as C

import numpy as np
import pytest

from lifcal_amd import _capi as capi


@pytest.fixture(scope="module")
def lib(built):
    return capi.load_library()


def test_new_symbols_are_exported(lib):
    for name in ("lifcal_ba_residual_report", "lifcal_ba_residual_groups", "lifcal_group_index", "lifcal_write_group_stats_csv"):
        assert hasattr(lib, name), name
    assert "lifcal_ba_residual_report" in capi.PROTOTYPES and "lifcal_ba_residual_groups" in capi.PROTOTYPES
    assert "lifcal_write_group_stats_csv" in capi.IO_PROTOTYPES


def test_group_stats_row_is_64_bytes_in_ctypes_and_numpy():
    assert C.sizeof(capi.GroupStats) == 64
    dt = capi.GROUP_STATS_DTYPE
    assert dt.itemsize == 64
    assert list(dt.names) == [f[0] for f in capi.GroupStats._fields_]
    for name in dt.names:
        assert dt.fields[name][1] == getattr(capi.GroupStats, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(capi.GroupStats, name).size, name


def group_index(lib, key, n_keys):
    key = np.ascontiguousarray(key, np.uint32)
    off = np.full(n_keys + 1, 0xFFFFFFFF, np.uint32); idx = np.full(len(key), 0xFFFFFFFF, np.uint32)
    rc = lib.lifcal_group_index(len(key), n_keys, capi.as_uptr(key), capi.as_uptr(off), capi.as_uptr(idx))
    return rc, off, idx


def test_group_index_of_nothing(lib):
    rc, off, idx = group_index(lib, np.zeros(0, np.uint32), 3)
    assert rc == 0 and np.array_equal(off, [0, 0, 0, 0]) and len(idx) == 0
    off0 = np.full(1, 7, np.uint32)
    assert lib.lifcal_group_index(0, 0, None, capi.as_uptr(off0), None) == 0 and off0[0] == 0


def test_group_index_one_key_holds_everything(lib):
    rc, off, idx = group_index(lib, np.zeros(37, np.uint32), 1)
    assert rc == 0 and np.array_equal(off, [0, 37]) and np.array_equal(idx, np.arange(37))


def test_group_index_with_empty_groups_between_used_ones(lib):
    key = np.array([5, 0, 5, 2, 0, 5], np.uint32)
    rc, off, idx = group_index(lib, key, 8)
    assert rc == 0
    assert np.array_equal(off, [0, 2, 2, 3, 3, 3, 6, 6, 6])
    assert np.array_equal(idx, [1, 4, 3, 0, 2, 5])


def test_group_index_rejects_a_key_out_of_range(lib):
    rc, _, _ = group_index(lib, np.array([0, 1, 4, 2], np.uint32), 4)
    assert rc == -1
    assert b"key[2]" in lib.lifcal_ba_last_error()
    off = np.zeros(5, np.uint32)
    assert lib.lifcal_group_index(4, 4, None, capi.as_uptr(off), None) == -1   # null key / idx with n > 0
    rc, off, idx = group_index(lib, np.array([0, 1, 3, 2], np.uint32), 4)       # and a valid call afterwards works
    assert rc == 0 and np.array_equal(idx, [0, 1, 3, 2])


def test_group_index_random_is_a_stable_sort(lib):
    rng = np.random.default_rng(7)
    n, n_keys = 5000, 97
    key = rng.integers(0, n_keys, n).astype(np.uint32)
    key[key == 13] = 14   # an empty group among used ones
    rc, off, idx = group_index(lib, key, n_keys)
    assert rc == 0
    assert np.array_equal(np.sort(idx), np.arange(n))   # a permutation
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_keys))]))
    assert off[13] == off[14]
    for k in range(n_keys):
        seg = idx[off[k]:off[k + 1]]
        assert np.all(key[seg] == k) and np.all(np.diff(seg.astype(np.int64)) > 0)
    assert np.array_equal(idx, np.argsort(key, kind="stable"))


def make_rows(rng, n):
    rows = np.zeros(n, capi.GROUP_STATS_DTYPE)
    cnt = rng.integers(1, 500, n).astype(np.uint32)
    rows["n"] = cnt
    rows["n_inliers"] = (cnt * rng.uniform(0, 1, n)).astype(np.uint32)
    for f in ("sum_x", "sum_y"):
        rows[f] = rng.normal(0, 1, n) * cnt
    for f in ("sum_xx", "sum_yy"):
        rows[f] = rng.uniform(0.01, 4, n) * cnt
    rows["sum_w"] = rng.uniform(0.1, 1, n) * cnt
    rows["max_abs_x"] = rng.uniform(0, 9, n); rows["max_abs_y"] = rng.uniform(0, 9, n)
    return rows


def read_csv(path):
    lines = open(path).read().splitlines()
    return lines[0].split(","), np.array([[float(x) for x in ln.split(",")] for ln in lines[1:]]).reshape(len(lines) - 1, -1)


def expected_columns(rows):
    n = rows["n"].astype(np.float64)
    return np.stack([n, rows["n_inliers"], rows["sum_x"] / n, rows["sum_y"] / n, np.sqrt(rows["sum_xx"] / n), np.sqrt(rows["sum_yy"] / n),
                     rows["max_abs_x"], rows["max_abs_y"], rows["sum_w"] / n], axis=1)


TAIL = ["n", "n_inliers", "mean_x", "mean_y", "rms_x", "rms_y", "max_abs_x", "max_abs_y", "mean_weight"]


def test_group_stats_csv_skips_empty_groups_and_round_trips(lib, tmp_path):
    rng = np.random.default_rng(3)
    rows = make_rows(rng, 9)
    rows[[0, 4, 8]] = np.zeros(1, capi.GROUP_STATS_DTYPE)   # empty groups: first, middle, last
    used = np.flatnonzero(rows["n"])
    ids = (np.arange(9) * 3 + 1).astype(np.int32)
    xy = rng.uniform(0, 4000, (9, 2))
    # all optional columns
    p = str(tmp_path / "a.csv")
    assert lib.lifcal_write_group_stats_csv(p.encode(), b"lens", 9, ids.ctypes.data_as(capi._iptr), capi.as_dptr(xy), rows.ctypes.data) == 0
    head, got = read_csv(p)
    assert head == ["lens", "x", "y"] + TAIL
    assert got.shape == (len(used), 12)
    assert np.array_equal(got[:, 0], ids[used])
    assert np.max(np.abs(got[:, 1:3] - xy[used])) <= 1e-6
    assert np.max(np.abs(got[:, 3:] - expected_columns(rows[used]))) <= 1e-6
    assert np.array_equal(got[:, 3], rows["n"][used]) and np.array_equal(got[:, 4], rows["n_inliers"][used])
    # no ids (the row index stands in), no centres
    p = str(tmp_path / "b.csv")
    assert lib.lifcal_write_group_stats_csv(p.encode(), b"point", 9, None, None, rows.ctypes.data) == 0
    head, got = read_csv(p)
    assert head == ["point"] + TAIL
    assert got.shape == (len(used), 10) and np.array_equal(got[:, 0], used)
    assert np.max(np.abs(got[:, 1:] - expected_columns(rows[used]))) <= 1e-6
    # nothing but the header for a table of empty groups; null arguments are rejected
    p = str(tmp_path / "c.csv")
    assert lib.lifcal_write_group_stats_csv(p.encode(), b"frame", 3, None, None, np.zeros(3, capi.GROUP_STATS_DTYPE).ctypes.data) == 0
    assert open(p).read().splitlines() == ["frame," + ",".join(TAIL)]
    assert lib.lifcal_write_group_stats_csv(None, b"frame", 0, None, None, None) == -1
    assert lib.lifcal_write_group_stats_csv(p.encode(), b"frame", 3, None, None, None) == -1


def test_store_residual_report_writes_the_three_files(lib, tmp_path):
    from lifcal_amd import GroupTable, ResidualReport, results
    rng = np.random.default_rng(5)
    fr, pt, ln = make_rows(rng, 4), make_rows(rng, 6), make_rows(rng, 5)
    pt[2] = np.zeros(1, capi.GROUP_STATS_DTYPE)
    lens_xy = rng.uniform(0, 2000, (5, 2))
    rep = ResidualReport(None, None, None, None, lens_xy, GroupTable(fr), GroupTable(pt), GroupTable(ln), GroupTable(make_rows(rng, 1)), 1.0, 0.0)
    results.storeResidualReport(str(tmp_path), [10, 11, 12, 13], rep)
    head, got = read_csv(tmp_path / "residualsPerFrame.csv")
    assert head[0] == "frame" and np.array_equal(got[:, 0], [10, 11, 12, 13]) and got.shape[1] == 10
    head, got = read_csv(tmp_path / "residualsPerPoint.csv")
    assert head[0] == "point" and np.array_equal(got[:, 0], [0, 1, 3, 4, 5])
    head, got = read_csv(tmp_path / "residualsPerLens.csv")
    assert head[:3] == ["lens", "x", "y"] and np.max(np.abs(got[:, 1:3] - lens_xy)) <= 1e-6
    assert np.max(np.abs(got[:, 5] - rep.per_lens.mean_x)) <= 1e-6 and np.max(np.abs(got[:, 11] - rep.per_lens.mean_weight)) <= 1e-6


def test_sensor_cells_cover_the_sensor():
    from lifcal_amd import sensor_cells
    u = np.array([0.0, 99.9, 100.0, 1023.9, -3.0, 5000.0]); v = np.array([0.0, 0.0, 150.0, 767.9, 10.0, 5000.0])
    key, n_keys, shape = sensor_cells(u, v, 100.0, 1024, 768)
    assert shape == (8, 11) and n_keys == 88 and key.dtype == np.uint32
    assert list(key) == [0, 0, 11 + 1, 7 * 11 + 10, 0, 87]
