"""EstimatorBatch with streams that are not in step (lmono_amd/host: per call the batch is the streams that are given a frame; each is, by its own
state, filling its window, initialising or running): streams that start late, stall, join a running batch and start over.  Host logic only -- the C ABI
is the CPU shim over the oracle (oracle/estimator_seq_cpu) -- so the bar is exact: under any schedule a stream prints, byte for byte, the lines of the
single-stream run of its file.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import estimator_stream as S
from tests.test_estimator_loop_cpu import _split_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "estimator_seq_cpu")
HOST = os.path.join(ROOT, "lmono_amd", "host")
LENGTHS = (48, 40, 33)


def _cpu_link(sources, exe, extra=()):
    """The g++ line of test_lockstep_loop_under_thread_sanitizer (the host mirror over the oracle shim), `extra` in the place of its -fsanitize=thread."""
    return (["g++", "-O1", "-g"] + list(extra) + ["-march=x86-64-v3", "-ffp-contract=off", "-std=c++17", "-pthread", "-I" + HOST, os.path.join(ROOT, "oracle", "cpu_shim.cpp"),
             os.path.join(HOST, "lmono_host.cpp")] + [os.path.join(HOST, f) for f in sources] + [os.path.join(HOST, "kitti_io.cpp"), os.path.join(ROOT, "oracle", "cpu_shim_stubs.o"),
             "-o", exe, "-L" + os.path.join(ROOT, "oracle"), "-llmono_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lm"])


def make_files(tmp_path, lengths=LENGTHS):
    """Three stream files of different lengths; the first and the last hold static stretches and a loop event."""
    from workloads import s2
    files = []
    for k, (n, seed, stops, loop_at) in enumerate(zip(lengths, (2, 0, 3), ((20, 21, 30), (), (25,)), (30, None, 28))):
        st = s2.make_stream(n, seed=seed, stops=stops)
        loops = [S.loop_event(st, loop_at)] if loop_at is not None else []
        for e in loops:                         # (a fixed corrected pose: the event needs no live window here)
            e["correct_T"] = np.array([0.1 * k, 0.2, 0.3]); e["correct_Q"] = np.array([1.0, 0.0, 0.001, 0.0])
        fx = tmp_path / ("s%d.bin" % k)
        S.write_stream(fx, st, loops)
        files.append(str(fx))
    return files


def single_runs(exe, files, *args):
    """-> per file (its lines without TIM / FLP / DIG, its digest)"""
    res = []
    for fx in files:
        out = subprocess.run([exe, fx, "-"] + list(args), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        res.append(([ln for ln in lines if not ln.startswith(("TIM", "FLP", "DIG"))], [ln.split()[2] for ln in lines if ln.startswith("DIG")][0]))
    return res


def run_schedule(exe, files, args, env=None):
    out = subprocess.run([exe, files[0], "-"] + list(args) + files[1:], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return _split_streams(out.stdout) + (out.stdout,)


def assert_every_stream_is_its_single_run(by, dig, single, n_streams, what):
    assert sorted(by) == list(range(n_streams)) and sorted(dig) == list(range(n_streams))
    for s in range(n_streams):
        lines, digest = single[s % len(single)]
        assert by[s] == lines, "%s: stream %d differs from the single-stream run of its file" % (what, s)
        assert dig[s] == digest, "%s: stream %d: digest" % (what, s)


def classes_by_tick(by, ticks_of):
    """{tick: set of classes} from the FRM lines' stage column (the stage AFTER the frame): fill while it is 0, init on the frame that turns it to 1,
    run behind it.  ticks_of(s) -> the tick of every frame of stream s."""
    at = {}
    for s, lines in by.items():
        stage = [int(ln.split()[3]) for ln in lines if ln.startswith("FRM")]
        ticks = ticks_of(s)
        assert len(ticks) >= len(stage)
        for f, st in enumerate(stage):
            c = "fill" if st == 0 else ("init" if f > 0 and stage[f - 1] == 0 else "run")
            at.setdefault(ticks[f], set()).add(c)
    return at


def schedule_ticks(start, stalls, n_frames):
    """The tick of every frame of a stream that starts at `start` and is away for the ticks [t0, t1) of `stalls` (frames are delayed, not dropped)."""
    ticks, t = [], start
    while len(ticks) < n_frames:
        if not any(t0 <= t < t1 for t0, t1 in stalls):
            ticks.append(t)
        t += 1
    return ticks


@pytest.fixture(scope="module")
def cpu_case(oracle, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "estimator_seq_cpu"])
    files = make_files(tmp_path_factory.mktemp("async_cpu"))
    return files, single_runs(EXE, files)


def test_staggered_start(cpu_case):
    """streams=5 start=7: stream s gets its first frame at tick 7 s, so the batch holds streams that fill, initialise and run at once."""
    files, single = cpu_case
    assert len({d for _, d in single}) == 3
    for mode in ("sync", "async"):
        by, dig, _ = run_schedule(EXE, files, [mode, "streams=5", "start=7"], env=dict(os.environ, LMONO_HOST_THREADS="3"))
        assert_every_stream_is_its_single_run(by, dig, single, 5, mode)
        at = classes_by_tick(by, lambda s: [7 * s + f for f in range(LENGTHS[s % 3])])
        mixed = [t for t, c in at.items() if c == {"fill", "init", "run"}]
        assert mixed, "the schedule must hold a tick with a filling, an initialising and a running stream"


def test_stalls(cpu_case):
    """Stream 1 (starts at tick 7) is away for 5 ticks while it fills its window and for 3 ticks while INITED (it initialises at tick 22); stream 2
    (starts at tick 14, would initialise at tick 24) is away across that tick.  Frames are delayed, not dropped."""
    files, single = cpu_case
    stall = "stall=1:10:15,1:30:33,2:22:26"
    for mode in ("sync", "async"):
        by, dig, _ = run_schedule(EXE, files, [mode, "streams=5", "start=7", stall], env=dict(os.environ, LMONO_HOST_THREADS="3"))
        assert_every_stream_is_its_single_run(by, dig, single, 5, mode + " " + stall)
    # the stalls fall where the docstring says: frame 10 is the initialisation frame of every file (the single runs' stage column) ...
    for lines, _ in single:
        stage = [int(ln.split()[3]) for ln in lines if ln.startswith("FRM")]
        assert stage[:10] == [0] * 10 and stage[10] == 1
    # ... and stream 1's next frame is frame 3 when it stalls first (filling) and frame 18 when it stalls again (INITED since frame 10), stream 2's is frame 8
    # when it stalls, so its frame 10 moves from tick 24 to tick 28
    t1 = schedule_ticks(7, [(10, 15), (30, 33)], LENGTHS[1]); t2 = schedule_ticks(14, [(22, 26)], LENGTHS[2])
    assert t1[2] == 9 and t1[3] == 15 and t1[10] == 22 and t1[17] == 29 and t1[18] == 33
    assert t2[7] == 21 and t2[8] == 26 and t2[10] == 28 and 22 <= 14 + 10 < 26


def test_join_and_restart(cpu_case):
    """start=5 join: the batch is built with one stream and the others are added with addStream() at their start ticks; restart=0:30: stream 0 starts
    over before tick 30 (resetStream) and its lines are those of its second incarnation -- the single run of its file again."""
    files, single = cpu_case
    for mode in ("sync", "async"):
        by, dig, _ = run_schedule(EXE, files, [mode, "streams=5", "start=5", "join", "restart=0:30"], env=dict(os.environ, LMONO_HOST_THREADS="3"))
        assert_every_stream_is_its_single_run(by, dig, single, 5, mode)
    # join does not combine with several groups
    out = subprocess.run([EXE, files[0], "-", "streams=4", "start=5", "join", "groups=2"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "join" in out.stderr


def test_batch_api_program(oracle, tmp_path):
    """lmono_amd/host/batch_api_test.cpp over the CPU shim: an all-absent call is a no-op, no hook for an absent stream, addStream / resetStream between
    Begin and Finish throw, addStream beyond the capacity throws, ESTIMATE_LASER == 2 is refused on this link with the single Estimator's message."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "estimator_seq_cpu"])          # (cpu_shim_stubs.o, liblmono_oracle.so)
    exe = str(tmp_path / "batch_api_test")
    b = subprocess.run(_cpu_link(["batch_api_test.cpp"], exe), capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    said = out.stdout
    for what in ("an all-absent call is a no-op", "the hook is not called for an absent stream", "addStream between Begin and Finish throws",
                 "resetStream between Begin and Finish throws", "addStream beyond the capacity throws", "ESTIMATE_LASER == 2 is refused on this link"):
        assert "ok " + what in said, what
    assert said.rstrip().endswith("batch_api_test: all ok")


def test_staggered_schedule_under_thread_sanitizer(oracle, tmp_path):
    """The staggered schedule on the host threads of the frame loop (the pool over the streams of a tick, the marginalisation worker, two batches
    interleaved by one driving thread), built with -fsanitize=thread as test_lockstep_loop_under_thread_sanitizer builds it: no report, one digest."""
    from workloads import s2
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "estimator_seq_cpu"])
    exe = str(tmp_path / "eseq_tsan")
    b = subprocess.run(_cpu_link(["estimator_seq.cpp"], exe, extra=["-fsanitize=thread"]), capture_output=True, text=True)
    if b.returncode != 0 and ("tsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("no ThreadSanitizer runtime: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr[-2000:]
    fx = tmp_path / "s.bin"
    s2.write_stream(str(fx), s2.make_stream(24, seed=2, stops=()))
    env = dict(os.environ, LMONO_HOST_THREADS="4", TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    out = subprocess.run([exe, str(fx), "-", "async", "streams=8", "start=3", "groups=2", "digest"], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr, out.stderr[-3000:]
    digs = [ln.split()[2] for ln in out.stdout.splitlines() if ln.startswith("DIG")]
    assert len(digs) == 8 and len(set(digs)) == 1
