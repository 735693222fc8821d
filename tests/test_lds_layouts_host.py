"""The dynamic-LDS layouts of csrc/mppi_lds.hpp on the host: tests/host_emul/lds_layouts.cpp (g++, no GPU) walks every
layout over T in 1..70, 255, 1000 and the control widths, filter windows, worlds and switches each takes, and this module
asserts for every case that

  (i)   the regions lie in the order the kernel carves them, do not overlap, and the last one ends at floats();
  (ii)  every region a kernel reads as float4 starts at a multiple of 4 floats;
  (iii) floats() is what the launch site computed BEFORE the layouts had one owner.  Those formulas are restated below from
        the launch sites of the commit before mppi_lds.hpp existed (capi_solve.hip, capi_search.hip, mppi_topk.hpp), not from
        the header: they are the independent statement.

The same program, built with -fsanitize=address,undefined, walks all layouts once as a stand-alone process."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "lds_layouts.cpp")
MAX_DIM_STATE, SUMMARY_HEAD = 8, 4  # include/mppi_hip.h


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lds_layouts") / "lds_layouts")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", path, SRC])
    return path


def records(exe, layout, ncols):
    raw = subprocess.run([exe, layout], capture_output=True, check=True).stdout
    rec = np.frombuffer(raw, np.int64)
    assert rec.size and rec.size % ncols == 0
    return rec.reshape(-1, ncols)


def check_regions(rec, first, total, float4=()):
    """(i) and (ii) for the {offset, size} pairs from column `first` on; `total`: where the last one must end."""
    off, size = rec[:, first::2], rec[:, first + 1::2]
    assert off.shape == size.shape and off.shape[1] >= 1
    assert (size >= 0).all() and (off[:, 0] == 0).all()
    assert (off[:, 1:] == off[:, :-1] + size[:, :-1]).all()  # in order, back to back: no overlap, no hole
    assert (off[:, -1] + size[:, -1] == total).all()
    for r in float4:
        assert (off[:, r] % 4 == 0).all()


def sg_staging(T, dc, window):  # `(sg_window ? (size_t)(2 * h->d.T - 1 + 2 * (sg_window / 2)) * h->dc : 0)`
    return np.where(window != 0, (2 * T - 1 + 2 * (window // 2)) * dc, 0)


def test_sweep_is_the_one_the_layouts_are_held_to(exe):
    rec = records(exe, "finalize", 15)
    T, dc, world, fold, w = (rec[:, i] for i in range(5))
    assert set(T) == set(range(1, 71)) | {255, 1000}
    assert set(dc) == {1, 2, 3, 4, 8, 64} and set(world) == {1, 2, 3, 8} and set(fold) == {0, 1}
    for t in (1, 2, 64, 1000):  # 0, then every odd window up to the widest mppi_set_sg_filter admits
        assert sorted(set(w[T == t])) == [0] + list(range(3, min(255, 2 * (2 * t - 1) + 1) + 1, 2))


def test_rollout(exe):
    rec = records(exe, "rollout", 19)
    T, dc, krow, ac, R, row, floats = (rec[:, i] for i in range(7))
    assert set(dc) == {1, 2, 4} and set(krow) == {0, 8} and set(ac) == {0, 1}
    assert (row == T * dc).all() and (R == (row + 3) // 4).all()
    lanes, rider = rec[:, 7:15], rec[:, 15:19]
    end_lanes = lanes[:, -2] + lanes[:, -1]
    end_rider = rider[:, -2] + rider[:, -1]
    check_regions(rec[:, :15], 7, end_lanes, float4=(0, 1, 2, 3))
    check_regions(np.concatenate([rec[:, :7], rider], axis=1), 7, end_rider)
    assert (floats == np.maximum(end_lanes, end_rider)).all()  # one launch serves both kinds of block
    # std::max((size_t)(term ? 12 : 8) * R + (size_t)T * KROW, (size_t)row + MPPI_MAX_DIM_STATE)
    assert (floats == np.maximum(np.where(ac != 0, 12, 8) * R + T * krow, row + MAX_DIM_STATE)).all()
    tight = (T == 1) & (krow == 0) & (ac == 0)  # one group, no step rows, no term: 8 < row + 8, the rider decides
    assert tight.any() and (end_rider[tight] > end_lanes[tight]).all()


def test_fused(exe):
    rec = records(exe, "fused", 19)
    T, dc, krow, w, R, row, floats = (rec[:, i] for i in range(7))
    check_regions(rec, 7, floats, float4=(0, 1, 2))
    # (size_t)8 * R + (size_t)T * KROW + 2 * (size_t)row + MPPI_SUMMARY_HEAD + (sg.window ? ... * h->dc : 0)
    assert (floats == 8 * R + T * krow + 2 * row + SUMMARY_HEAD + sg_staging(T, dc, w)).all()


def test_finalize(exe):
    rec = records(exe, "finalize", 15)
    T, dc, world, fold, w, row, floats = (rec[:, i] for i in range(7))
    check_regions(rec, 7, floats)
    # (size_t)row + (size_t)world * (row + MPPI_SUMMARY_HEAD) + (sg_window ? ... : 0) + (fold ? (SUM_BLOCK / SUM_COLS) * (row + 3) : 0)
    assert (floats == row + world * (row + SUMMARY_HEAD) + sg_staging(T, dc, w) + np.where(fold != 0, (1024 // 16) * (row + 3), 0)).all()


def test_state_seq(exe):
    rec = records(exe, "state_seq", 8)
    row, floats = rec[:, 2], rec[:, 3]
    check_regions(rec, 4, floats)
    assert (floats == row + MAX_DIM_STATE).all()  # sizeof(float) * ((size_t)h->d.row + MPPI_MAX_DIM_STATE)


def test_wave_rollout(exe):
    rec = records(exe, "wave", 21)
    T, dc, ds, R, floats = (rec[:, i] for i in range(5))
    assert set(ds) == {2, 3, 4, 7}
    check_regions(rec, 5, floats)
    assert (floats == 4 * (4 * R + (T + 1) * ds)).all()  # sizeof(float) * 4 * ((size_t)4 * R + (size_t)(T + 1) * DS)


def test_topk(exe):
    rec = records(exe, "topk", 12)
    T, dc, srt, gen, R, floats = (rec[:, i] for i in range(6))
    check_regions(rec, 6, floats, float4=(0, 1, 2))
    # sizeof(float) * 8 * (size_t)R + (!sorted && gen_noise && R <= TOPK_PREGEN_MAX_R ? sizeof(float4) * 64 * (size_t)R : 0)
    nbytes = 4 * 8 * R + np.where((srt == 0) & (gen != 0) & (R <= 32), 16 * 64 * R, 0)
    assert (4 * floats == nbytes).all()
    assert ((srt == 0) & (gen != 0) & (R == 32)).any() and ((srt == 0) & (gen != 0) & (R == 33)).any()  # both sides of the limit


def test_brent_staging(exe):
    rec = records(exe, "brent", 5)
    check_regions(rec, 3, rec[:, 2])
    assert (rec[:, 2] == rec[:, 0] * rec[:, 1]).all()  # sizeof(float) * (size_t)per_thread * threads


def test_standalone_program_passes_the_sanitizers(tmp_path):
    san = str(tmp_path / "lds_layouts_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, SRC])
    out = subprocess.run([san, "all"], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert len(out.stdout) % 8 == 0 and len(out.stdout) > 0
