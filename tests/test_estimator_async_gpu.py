"""EstimatorBatch with streams that are not in step, on the GPU (lmono_amd/host/estimator_seq; the schedules of tests/test_estimator_async_cpu.py):
per tick the numeric calls run over the windows of the streams that need them, so the number of windows in a call changes from tick to tick -- and a
window's bytes must not depend on the batch it travels in.  The bar is exact: every stream prints the lines of the single-stream run of its file, made
on the device too.  ESTIMATE_LASER == 2 streams calibrate inside the batch, in step and out of step."""
import os

import pytest

from tests import test_estimator_async_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmono_amd", "host", "estimator_seq")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def three_files(tmp_path_factory):
    files = A.make_files(tmp_path_factory.mktemp("async_gpu"))
    return files, A.single_runs(EXE, files)


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_staggered_start_with_stalls(three_files, mode):
    """streams=6 start=7 with the three stalls of the CPU test: fill, init and run streams in one tick, a stream away while it fills, while INITED and
    across its initialisation tick; files of 48, 40 and 33 frames, so the batch also shrinks as streams run out."""
    files, single = three_files
    stall = "stall=1:10:15,1:30:33,2:22:26"
    by, dig, _ = A.run_schedule(EXE, files, [mode, "streams=6", "start=7", stall])
    A.assert_every_stream_is_its_single_run(by, dig, single, 6, mode + " " + stall)
    ticks = {0: A.schedule_ticks(0, [], 48), 1: A.schedule_ticks(7, [(10, 15), (30, 33)], 40), 2: A.schedule_ticks(14, [(22, 26)], 33),
             3: A.schedule_ticks(21, [], 48), 4: A.schedule_ticks(28, [], 40), 5: A.schedule_ticks(35, [], 33)}
    at = A.classes_by_tick(by, lambda s: ticks[s])
    assert [t for t, c in at.items() if c == {"fill", "init", "run"}], "the schedule must hold a tick with a filling, an initialising and a running stream"


@pytest.fixture(scope="module")
def one_file(tmp_path_factory):
    from workloads import s2
    fx = tmp_path_factory.mktemp("async_gpu_ramp") / "s40.bin"
    s2.write_stream(str(fx), s2.make_stream(40, seed=2, stops=(20, 21)))
    return [str(fx)], A.single_runs(EXE, [str(fx)])


@pytest.mark.parametrize("cluster", [None, "1"])
def test_window_count_ramps_across_the_cluster_boundary(one_file, cluster):
    """streams=10 start=1: stream s solves from tick s + 10 (its frame 10) to tick s + 39, so the solve call holds 1, 2, ... 10 windows at ticks 10 .. 19 --
    across 8 -> 9, where the launch grows by a second group of eight clusters -- and 9 ... 1 at the end.  Every digest is the single run's, with the
    default workgroups per window and with one (LMONO_BA_CLUSTER=1)."""
    files, single = one_file
    lines, digest = single[0]
    stage = [int(ln.split()[3]) for ln in lines if ln.startswith("FRM")]
    assert len(stage) == 40 and stage[:10] == [0] * 10 and all(v == 1 for v in stage[10:])
    windows = [sum(1 for s in range(10) if s + 10 <= t <= s + 39) for t in range(49)]
    assert windows[10:20] == list(range(1, 11)) and windows[17:19] == [8, 9] and windows[40:49] == list(range(9, 0, -1))
    env = dict(os.environ) if cluster is None else dict(os.environ, LMONO_BA_CLUSTER=cluster)
    by, dig, out = A.run_schedule(EXE, files, ["streams=10", "start=1", "digest"], env=env)
    assert by == {} and sorted(dig) == list(range(10))
    assert [dig[s] for s in range(10)] == [digest] * 10
    tim = [ln for ln in out.splitlines() if ln.startswith("TIM")][0].split()
    assert int(tim[1]) == 38                      # ticks 11 .. 48 launch the solve of an INITED stream


def _kinds(lines):
    return ([ln for ln in lines if ln.startswith("FRM")], [ln for ln in lines if ln.startswith("ODO")], [ln for ln in lines if ln.startswith("CAL")])


@pytest.fixture(scope="module")
def calib_files(tmp_path_factory):
    from workloads import s2, s7
    d = tmp_path_factory.mktemp("async_gpu_calib")
    files = []
    for name, st in (("handheld", s7.make_stream(25, seed=0, angle_deg=(8.0, 12.0))), ("yaw", s7.make_stream(25, seed=1, angle_deg=(8.0, 12.0), yaw_only=True))):
        fx = d / (name + ".bin")
        s2.write_stream(fx, st)
        files.append(str(fx))
    return files, A.single_runs(EXE, files, "estimate_laser=2")


def test_calibration_in_step(calib_files):
    """estimate_laser=2 streams=2 of the hand-held stream: one lmono_excalib_step per frame over both streams; both calibrate on frame 10, initialise in
    that frame and print the single run's CAL, FRM and ODO lines."""
    files, single = calib_files
    frm, odo, cal = _kinds(single[0][0])
    assert len(cal) == 1 and int(cal[0].split()[1]) == 10 and len(frm) == 25 and len(odo) == 15
    by, dig, _ = A.run_schedule(EXE, files[:1], ["estimate_laser=2", "streams=2"])
    A.assert_every_stream_is_its_single_run(by, dig, single[:1], 2, "in step")
    for s in range(2):
        assert _kinds(by[s]) == (frm, odo, cal)


def test_calibration_out_of_step(calib_files):
    """estimate_laser=2 streams=3 start=4: stream 0 (hand-held) calibrates and solves from tick 10 on while stream 2, the same file started at tick 8,
    still calibrates and stream 1 (yaw only, started at tick 4) never does and only slides its window."""
    files, single = calib_files
    by, dig, _ = A.run_schedule(EXE, files, ["estimate_laser=2", "streams=3", "start=4"])
    A.assert_every_stream_is_its_single_run(by, dig, single, 3, "out of step")
    frm0, odo0, cal0 = _kinds(by[0]); frm1, odo1, cal1 = _kinds(by[1]); frm2, odo2, cal2 = _kinds(by[2])
    assert [int(ln.split()[3]) for ln in frm0] == [0] * 10 + [1] * 15 and len(cal0) == 1 and cal0 == cal2 and odo0 == odo2 and len(odo0) == 15
    assert len(frm1) == 25 and cal1 == [] and odo1 == [] and all(int(ln.split()[3]) == 0 for ln in frm1)
    # stream 0 initialises at tick 10 and runs to tick 24 beside streams that only fill or slide (stream 2 at its frames 2 .. 9 until tick 17, stream 1)
    at = A.classes_by_tick(by, lambda s: [4 * s + f for f in range(25)])
    assert at[10] == {"init", "fill"} and all(at[t] == {"run", "fill"} for t in range(11, 18))
