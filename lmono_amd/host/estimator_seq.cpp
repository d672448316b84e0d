// lmono_amd/host/estimator_seq.cpp -- replays a frame stream through the host mirror's Estimator::processImage (the reference's
// processEstimation without ROS and the image tracker, Estimator.cc:528-553) and prints, per frame, what the Python tests compare
// with the CPU oracle, then the trajectory of record in the reference's new_odometry.txt format (Estimator.cc:642-644).
//
// Stream file (doubles): n_frames, TLC[16], then per frame: header, L0_Pos[16], n_loop (0/1) [loop_time_stamp, old_T[3],
// old_Q[4] w x y z, correct_T[3], correct_Q[4] w x y z], n_features, n_features x (id, x_n, y_n, u, v).
// Usage: estimator_seq <stream.bin> [new_odometry.txt | -] [sync | async] [estimate_laser=K]
//                      [streams=N [groups=G] [digest] [start=K [join]] [stall=S:T0:T1[,...]] [restart=S:T[,...]] [more stream files ...]]
// "estimate_laser=K": Params::ESTIMATE_LASER (default 1).  With 2 a stream finds the camera-LiDAR rotation by hand-eye calibration
// (Estimator.cc:403-430) and prints one "CAL <frame> <rlc, 9 numbers row-major>" line behind the FRM line of the frame it succeeds on
// (streams=N: the batch calibrates its streams in one lmono_excalib_step per frame; the CAL line comes from the frame hook).
// "async": marginalisation overlapped with the next frame (Estimator::setAsyncMargin); the PRI line (digest of the last prior) and
// everything else must come out the same bytes as without it.
// "streams=N": N independent Estimators stepped by EstimatorBatch (one batched C-ABI call per numeric step); stream s replays
// file s mod (number of files given).  Every stream's lines are printed behind a "STR s" line and are, byte for byte, the lines of the
// single-stream run of its file (and "DIG s <hash>" = FNV-1a of those lines; "digest": print only the DIG lines -- 256 streams x 2761 frames
// of text is 70 MB).  The single-stream run prints its own "DIG 0 <hash>" over the same lines.
// The run goes tick by tick; per tick every stream is given its next frame unless the schedule keeps it away, and the files may hold different numbers
// of frames: a stream that has run out stays away, the run ends when every stream has.  Without the arguments below all streams are in step.
//   "start=K": stream s gets its first frame at tick s * K.    "join" (with start=): stream s > 0 is not built up front but added with
//   EstimatorBatch::addStream() at its start tick (not with groups > 1).
//   "stall=S:T0:T1": stream S is away for the ticks T0 <= t < T1; its frames are delayed, not dropped.
//   "restart=S:T": before tick T, EstimatorBatch::resetStream(S); the stream goes back to frame 0 of its file and its lines and digest start again.
// "TIM n ms N G": n = the ticks that launched the solve of an INITED stream, ms = their mean wall time.
// "groups=G": the N streams as G EstimatorBatches of N / G streams, each on its own context (own HIP stream).  ONE thread interleaves the groups --
// finish(g, tick t - 1), begin(g, tick t) for g = 0 .. G - 1 -- so that one group's host passes run beside another group's solve (the sequences are
// independent); whether a tick counts for TIM is sampled before the pending Finish, so with G > 1 the count is off by one around the initialisation
// frame.  Three or more groups need LMONO_BA_CLUSTER=1: every context sizes its clusters of workgroups per window for a chip of its own, so the budgets
// of three contexts together can oversubscribe the CUs, and a cluster that is not resident as a whole gives up and is solved again.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "lmono_host.hpp"

using namespace lmono_host;

static std::vector<double> read_all(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    std::vector<double> v((size_t)n / 8);
    if (std::fread(v.data(), 8, v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

struct Frame {
    double header; double L0[16];
    bool has_loop = false; Estimator::LoopFrame loop;
    FeatureManager::Image image;
};
struct Stream { double TLC[16]; std::vector<Frame> frames; };

static Stream parse_stream(const char *path)
{
    const std::vector<double> d = read_all(path);
    size_t k = 0;
    Stream st;
    const int n_frames = (int)d[k++];
    for (int j = 0; j < 16; j++) st.TLC[j] = d[k++];
    st.frames.resize((size_t)n_frames);
    for (int f = 0; f < n_frames; f++) {
        Frame &fr = st.frames[(size_t)f];
        fr.header = d[k++];
        for (int j = 0; j < 16; j++) fr.L0[j] = d[k++];
        if ((int)d[k++]) {
            fr.has_loop = true;
            Estimator::LoopFrame &lf = fr.loop;
            lf.loop_time_stamp = d[k++];
            for (int j = 0; j < 3; j++) lf.old_T[j] = d[k++];
            for (int j = 0; j < 4; j++) lf.old_Q[j] = d[k++];
            for (int j = 0; j < 3; j++) lf.correct_T[j] = d[k++];
            for (int j = 0; j < 4; j++) lf.correct_Q[j] = d[k++];
        }
        const int nf = (int)d[k++];
        for (int j = 0; j < nf; j++) { const int id = (int)d[k]; fr.image[id] = { d[k + 1], d[k + 2], d[k + 3], d[k + 4] }; k += 5; }
    }
    return st;
}

// the lines of one stream (FRM per frame, then ODO / PRI / EXT) and their running digest
struct Lines {
    std::string text;
    unsigned long long h = 1469598103934665603ull;
    bool keep = true;
    void add(const char *s)
    {
        for (const char *p = s; *p; p++) { h ^= (unsigned char)*p; h *= 1099511628211ull; }
        if (keep) text += s;
    }
};
static void frm_line(Lines &out, int f, bool keyframe, const Estimator &est)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, "FRM %d %d %d %d %d %d %.17g %d %d %zu\n", f, keyframe ? 1 : 0, (int)est.stage_flag, est.static_status ? 1 : 0, est.iterations, est.termination,
                  est.final_cost, est.margin_calls[0], est.margin_calls[1], est.feature_manager.feature.size());
    out.add(buf);
}
static void cal_line(Lines &out, size_t f, const Estimator &est)
{
    std::string c = "CAL " + std::to_string(f);
    char buf[64];
    for (int j = 0; j < 9; j++) { std::snprintf(buf, sizeof buf, " %.17g", est.calib_rlc[j]); c += buf; }
    c += "\n";
    out.add(c.c_str());
}
static void tail_lines(Lines &out, const Estimator &est)
{
    char buf[1024];
    for (const auto &r : est.new_odometry) {
        std::snprintf(buf, sizeof buf, "ODO %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
        out.add(buf);
    }
    const auto &mi = est.last_marginalization_info;
    double sj = 0, sr = 0;
    for (double v : mi.linearized_jacobians) sj += v * v;
    for (double v : mi.linearized_residuals) sr += v * v;
    std::snprintf(buf, sizeof buf, "PRI %d %d %d %zu %.17g %.17g\n", mi.m, mi.n, mi.status, mi.parameter_blocks.size(), sj, sr);
    out.add(buf);
    std::string e = "EXT";
    for (int j = 0; j < 16; j++) { std::snprintf(buf, sizeof buf, " %.17g", est.TLC[j]); e += buf; }
    e += "\n";
    out.add(e.c_str());
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        int n_streams = 0, n_groups = 1, estimate_laser = -1, start_every = 0; bool digest_only = false, async = false, join = false;
        std::vector<std::array<long, 3>> stalls, restarts;       // stream, first tick, end tick | stream, tick
        // "S:T0:T1,S:T0:T1 ..." (fields = 3) or "S:T,..." (fields = 2)
        auto parse_list = [](const char *txt, int fields, std::vector<std::array<long, 3>> &to) {
            const char *c = txt;
            while (*c) {
                std::array<long, 3> v{ { 0, 0, 0 } };
                for (int k = 0; k < fields; k++) {
                    char *end = nullptr;
                    v[(size_t)k] = std::strtol(c, &end, 10);
                    if (end == c || (k + 1 < fields && *end != ':')) return false;
                    c = k + 1 < fields ? end + 1 : end;
                }
                to.push_back(v);
                if (*c == ',') c++; else if (*c) return false;
            }
            return true;
        };
        std::vector<const char *> files{ argv[1] };
        for (int a = 3; a < argc; a++) {
            const std::string s = argv[a];
            if (s == "async") async = true;
            else if (s == "sync") async = false;
            else if (s.rfind("estimate_laser=", 0) == 0) estimate_laser = std::atoi(s.c_str() + 15);
            else if (s.rfind("streams=", 0) == 0) n_streams = std::atoi(s.c_str() + 8);
            else if (s.rfind("groups=", 0) == 0) n_groups = std::max(1, std::atoi(s.c_str() + 7));
            else if (s == "digest") digest_only = true;
            else if (s.rfind("start=", 0) == 0) start_every = std::max(0, std::atoi(s.c_str() + 6));
            else if (s == "join") join = true;
            else if (s.rfind("stall=", 0) == 0) { if (!parse_list(s.c_str() + 6, 3, stalls)) { std::fprintf(stderr, "estimator_seq: stall=S:T0:T1[,...]\n"); return 2; } }
            else if (s.rfind("restart=", 0) == 0) { if (!parse_list(s.c_str() + 8, 2, restarts)) { std::fprintf(stderr, "estimator_seq: restart=S:T[,...]\n"); return 2; } }
            else files.push_back(argv[a]);
        }
        HipContext hip(0);
        Params p;
        if (estimate_laser >= 0) {
            if (estimate_laser > 2) { std::fprintf(stderr, "estimator_seq: estimate_laser is 0, 1 or 2\n"); return 2; }
            p.ESTIMATE_LASER = estimate_laser;
        }
        if (n_streams <= 0) {
            const Stream st = parse_stream(argv[1]);
            Estimator est(hip, p);
            if (async) est.setAsyncMargin(true);
            std::memcpy(est.TLC, st.TLC, sizeof(st.TLC));
            Lines out;
            double solve_ms = 0; int solves = 0;
            for (size_t f = 0; f < st.frames.size(); f++) {
                const Frame &fr = st.frames[f];
                if (fr.has_loop) est.setLoopFrame(fr.loop);
                const bool was_inited = est.stage_flag == Estimator::INITED, was_calibrated = est.extrinsic_calibrated;
                const auto t0 = std::chrono::steady_clock::now();
                const bool keyframe = est.processImage(fr.header, fr.image, fr.L0);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (was_inited) { solve_ms += ms; solves++; }
                frm_line(out, (int)f, keyframe, est);
                if (est.extrinsic_calibrated && !was_calibrated) cal_line(out, f, est);
            }
            est.marginWait();
            tail_lines(out, est);
            std::fputs(out.text.c_str(), stdout);
            std::printf("DIG 0 %016llx\n", out.h);
            std::printf("TIM %d %.6f\n", solves, solves ? solve_ms / solves : 0.0);
            std::printf("FLP %.17g %ld\n", est.solve_flops, est.solve_obs);     // algorithmic flops of all window solves, projection blocks in all
            lmono_host::estimator_print_phase_clock();
            if (argc > 2 && std::string(argv[2]) != "-") {
                FILE *fo = std::fopen(argv[2], "w");
                if (!fo) { std::perror(argv[2]); return 2; }
                for (const auto &r : est.new_odometry) std::fprintf(fo, "%f %f %f %f %f %f %f %f\n", r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);   // Estimator.cc:642
                std::fclose(fo);
            }
            return 0;
        }
        // ---- N streams in one or more EstimatorBatches, tick by tick: per tick a stream is given its next frame unless the schedule keeps it away
        if (join && n_groups > 1) { std::fprintf(stderr, "estimator_seq: join cannot be combined with groups > 1\n"); return 2; }
        if (join && start_every <= 0) { std::fprintf(stderr, "estimator_seq: join needs start=K\n"); return 2; }
        std::vector<Stream> src;
        for (const char *f : files) src.push_back(parse_stream(f));
        const int N = n_streams, G = std::min(n_groups, N);
        for (const auto &st : stalls) if (st[0] < 0 || st[0] >= N) { std::fprintf(stderr, "estimator_seq: stall names no stream\n"); return 2; }
        for (const auto &rs : restarts) if (rs[0] < 0 || rs[0] >= N) { std::fprintf(stderr, "estimator_seq: restart names no stream\n"); return 2; }
        std::vector<Lines> out((size_t)N);
        for (int s = 0; s < N; s++) out[(size_t)s].keep = !digest_only;
        // per stream: the next frame of its file, the frame it is working on (the frame hook prints it), whether its CAL line has been printed
        std::vector<size_t> pos((size_t)N, 0), cur_f((size_t)N, 0);
        std::vector<char> calibrated((size_t)N, 0), given((size_t)N, 0);
        auto file_of = [&](int s) -> const Stream & { return src[(size_t)s % src.size()]; };
        // the schedule: is stream s away at tick t (not started yet, or stalled)?
        auto away = [&](int s, long t) {
            if (t < (long)s * start_every) return true;
            for (const auto &st : stalls) if (st[0] == s && t >= st[1] && t < st[2]) return true;
            return false;
        };
        // group g: streams [s0, s0 + n) as one EstimatorBatch on its own context / HIP stream (G = 1: the context above).  ONE thread drives all groups, tick by
        // tick: finish(g, tick t - 1), begin(g, tick t) for g = 0 .. G - 1 -- a group's solve is in flight while the thread runs the other groups' host
        // passes (threads per group were measured first: the HIP runtime serialises the submitting threads, 9.1 -> 10.4 ms per lock-step frame at G = 2)
        struct Group {
            int s0 = 0, n = 0, cap = 0;   // n: streams constructed so far (join: they are added at their start ticks)
            std::unique_ptr<HipContext> own;
            std::unique_ptr<EstimatorBatch> eb;
            std::vector<double> headers;
            std::vector<const FeatureManager::Image *> img;
            std::vector<std::array<double, 16>> L0;
            std::unique_ptr<bool[]> kf;
        };
        std::vector<Group> grp((size_t)G);
        for (int g = 0; g < G; g++) {
            Group &q = grp[(size_t)g];
            q.s0 = (int)((long long)g * N / G); q.cap = (int)((long long)(g + 1) * N / G) - q.s0;
            q.n = join ? 1 : q.cap;
            if (G > 1) { q.own.reset(new HipContext(0)); q.own->useOwnStream(); }
            q.eb.reset(new EstimatorBatch(G > 1 ? *q.own : hip, p, q.n, 0, q.cap));
            if (async) q.eb->setAsyncMargin(true);
            for (int s = 0; s < q.n; s++) std::memcpy(q.eb->stream(s).TLC, file_of(q.s0 + s).TLC, 128);
            q.headers.resize((size_t)q.cap); q.img.resize((size_t)q.cap); q.L0.resize((size_t)q.cap); q.kf.reset(new bool[(size_t)q.cap]);
            // a stream's FRM line (and its CAL line behind the frame it calibrates on) is written at the end of its frame by the thread that ran the stream's
            // last pass (EstimatorBatch::setFrameHook): no serial loop over the streams on the driving thread
            Group *qp = &q;
            q.eb->setFrameHook([qp, &out, &cur_f, &calibrated](int s, const Estimator &e) {
                const size_t gs = (size_t)(qp->s0 + s);
                frm_line(out[gs], (int)cur_f[gs], qp->kf[(size_t)s], e);
                if (e.extrinsic_calibrated && !calibrated[gs]) { calibrated[gs] = 1; cal_line(out[gs], cur_f[gs], e); }
            });
        }
        auto begin = [&](Group &q, long t) {
            for (int s = 0; s < q.cap; s++) {
                const int gs = q.s0 + s;
                const Stream &st = file_of(gs);
                for (const auto &rs : restarts) if (rs[0] == gs && rs[1] == t && s < q.n) {
                    Estimator &fresh = q.eb->resetStream(s);
                    std::memcpy(fresh.TLC, st.TLC, 128);
                    pos[(size_t)gs] = 0; calibrated[(size_t)gs] = 0;
                    out[(size_t)gs] = Lines(); out[(size_t)gs].keep = !digest_only;
                }
                if (s == q.n && join && t >= (long)gs * start_every) {           // joins at its start tick
                    const int k = q.eb->addStream();
                    std::memcpy(q.eb->stream(k).TLC, st.TLC, 128);
                    q.n++;
                }
                q.img[(size_t)s] = nullptr;
                if (s >= q.n || away(gs, t) || pos[(size_t)gs] >= st.frames.size()) continue;
                const Frame &fr = st.frames[pos[(size_t)gs]];
                cur_f[(size_t)gs] = pos[(size_t)gs]++;
                q.headers[(size_t)s] = fr.header; q.img[(size_t)s] = &fr.image; std::memcpy(q.L0[(size_t)s].data(), fr.L0, 128);
                if (fr.has_loop) q.eb->stream(s).setLoopFrame(fr.loop);
            }
            q.eb->processImageBegin(q.headers.data(), q.img.data(), reinterpret_cast<const double (*)[16]>(q.L0.data()), q.kf.get());
        };
        auto finish = [&](Group &q) { q.eb->processImageFinish(); };
        // the run ends when every stream has been given every frame of its file (a restart puts a stream back to its first)
        auto work_left = [&](long t) {
            for (int s = 0; s < N; s++) if (pos[(size_t)s] < file_of(s).frames.size()) return true;
            for (const auto &rs : restarts) if (rs[1] >= t) return true;
            return false;
        };
        double solve_ms = 0; int solves = 0;
        for (long t = 0; work_left(t); t++) {
            // TIM counts the ticks that launched a solve of an INITED stream: G = 1, a stream that is INITED now is given a frame in this tick; G > 1, the
            // iteration finishes tick t - 1, so: a stream that was given a frame in tick t - 1 and was INITED before it (sampled before the pending Finish)
            bool was_inited = false;
            for (int g = 0; g < G; g++) {
                Group &q = grp[(size_t)g];
                for (int s = 0; s < q.n; s++) {
                    const int gs = q.s0 + s;
                    if (q.eb->stream(s).stage_flag != Estimator::INITED) continue;
                    bool restarting = false;
                    for (const auto &rs : restarts) if (rs[0] == gs && rs[1] == t) restarting = true;
                    if (G > 1 ? given[(size_t)gs] != 0 : (!restarting && !away(gs, t) && pos[(size_t)gs] < file_of(gs).frames.size())) was_inited = true;
                }
            }
            const auto t0 = std::chrono::steady_clock::now();
            for (int g = 0; g < G; g++) {
                if (G > 1 && t > 0) finish(grp[(size_t)g]);
                begin(grp[(size_t)g], t);
                if (G == 1) finish(grp[(size_t)g]);
            }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            // (G > 1: an iteration finishes tick t - 1 and begins tick t of every group: one lock-step frame of work, counted when tick t - 1 held an INITED frame)
            if (G == 1 ? was_inited : (t > 0 && was_inited)) { solve_ms += ms; solves++; }
            if (G > 1) for (int g = 0; g < G; g++) for (int s = 0; s < grp[(size_t)g].cap; s++) given[(size_t)(grp[(size_t)g].s0 + s)] = grp[(size_t)g].img[(size_t)s] ? 1 : 0;
        }
        if (G > 1) for (int g = 0; g < G; g++) finish(grp[(size_t)g]);
        double flops = 0; long obs = 0;
        for (int g = 0; g < G; g++) {
            Group &q = grp[(size_t)g];
            q.eb->marginWait();
            for (int s = 0; s < q.n; s++) {
                tail_lines(out[(size_t)(q.s0 + s)], q.eb->stream(s));
                flops += q.eb->stream(s).solve_flops; obs += q.eb->stream(s).solve_obs;
            }
        }
        for (int s = 0; s < N; s++) {
            if (!digest_only) { std::printf("STR %d\n", s); std::fputs(out[(size_t)s].text.c_str(), stdout); }
            std::printf("DIG %d %016llx\n", s, out[(size_t)s].h);
        }
        grp.clear();          // (the batches print their phase clocks as they go)
        // TIM: lock-step frames timed (INITED), milliseconds per lock-step frame (= N stream frames), streams
        std::printf("TIM %d %.6f %d %d\n", solves, solves ? solve_ms / solves : 0.0, N, G);
        std::printf("FLP %.17g %ld\n", flops, obs);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "estimator_seq: %s\n", e.what());
        return 1;
    }
}
