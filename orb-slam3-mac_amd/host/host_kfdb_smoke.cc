// host_kfdb_smoke.cc -- flat-file driver of host/KeyFrameDatabase.cc (tests/test_kfdb_model.py, tests/test_gpu_kfdb.py):
//   host_kfdb_smoke run SCRIPT            the script through the class on the device
//   host_kfdb_smoke tail SCRIPT FEED      the same with the device call replaced by the lists in FEED (no GPU): the class's host tail
//   host_kfdb_smoke threads SCRIPT [FEED] the same with every second operation, the first included, made by a thread of its own that
//                                         ends right after it (as LoopClosing, Tracking and SetBadFlag's thread share one database);
//                                         without FEED a further thread keeps its own thread context busy with a small database of its
//                                         own all the while and checks every answer it gets
//   host_kfdb_smoke latency [KF WORDS VOCAB REPS]   wall time of one DetectNBestCandidates and one DetectRelocalizationCandidates call
// SCRIPT (text): "n n_slots n_maps", the maps' bad flags, per keyframe "map nwords (word value)* nneigh neigh*" (values as hex floats;
// keyframes at index >= n_slots never enter the database), "nops", then per line: add K | erase K | clear_map M | clear |
// nbest ID MAP NCAND nwords (word value)* nconn conn* | reloc ID MAP NCAND nwords (word value)* 0.
// FEED: per Detect... "n_sharing max_common n_scored n_touched" and n_sharing + n_touched rows "keyframe words scored score_bits".
// Output per operation: "op I", "loop ..", "merge ..", "reloc .." (keyframe indices) and per slotted keyframe its six fields
// "K PRquery PRwords PRscore_bits Rquery Rwords Rscore_bits".
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "KeyFrameDatabase.h"
#include "hip_context.h"

using namespace ORB_SLAM3;

namespace {

uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

bool read_bow(FILE *fp, DBoW2::BowVector &bow)
{
    int n = 0;
    if (fscanf(fp, "%d", &n) != 1) return false;
    for (int i = 0; i < n; i++) {
        int w; double v;
        if (fscanf(fp, "%d %la", &w, &v) != 2) return false;
        bow[(DBoW2::WordId)w] = v;
    }
    return true;
}

int fail(const char *what) { fprintf(stderr, "host_kfdb_smoke: %s\n", what); return 2; }

// what another thread of the process does meanwhile on ITS context: a 3-keyframe database, one query after the other, every answer checked
void busy_on_own_context(std::atomic<bool> &stop, std::atomic<long> &calls, std::atomic<int> &wrong)
{
    orbhip_ctx *ctx = hip::ThreadContext();
    orbhip_kfdb *db = nullptr;
    if (!ctx || orbhip_kfdb_create(ctx, 4, 8, &db) != ORBHIP_OK) { wrong = 1; return; }
    const int32_t w[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const double v[8] = {.125, .125, .125, .125, .125, .125, .125, .125};
    for (int s = 0; s < 3; s++) if (orbhip_kfdb_add_host(db, s, 0, w, v, 8) != ORBHIP_OK) wrong = 1;
    for (uint64_t id = 1; !stop.load(); id++) {
        orbhip_kfdb_query q; q.id = id; q.map_id = 0; q.mode = ORBHIP_KFDB_RELOC;
        int32_t counts[4]; orbhip_kfdb_entry list[4];
        const int rc = orbhip_kfdb_score_host(db, &q, w, v, 8, nullptr, 0, 4, counts, list);
        if (rc != ORBHIP_OK || counts[0] != 3 || counts[1] != 8 || counts[2] != 3 || counts[3] != 0) { wrong = 1; break; }
        for (int i = 0; i < 3; i++) if (list[i].slot != i || list[i].words != 8 || list[i].score != 1.0f) wrong = 1;
        calls++;
    }
    orbhip_kfdb_destroy(db);
}

int run_script(const char *script, const char *feed_path, bool threaded = false)
{
    FILE *fp = fopen(script, "r");
    if (!fp) return fail("cannot open the script");
    FILE *feed = feed_path ? fopen(feed_path, "r") : nullptr;
    if (feed_path && !feed) return fail("cannot open the feed");
    int n, n_slots, n_maps;
    if (fscanf(fp, "%d %d %d", &n, &n_slots, &n_maps) != 3) return fail("bad header");
    std::vector<Map *> maps;
    for (int m = 0; m < n_maps; m++) {
        int bad;
        if (fscanf(fp, "%d", &bad) != 1) return fail("bad map flags");
        maps.push_back(new Map());
        if (bad) maps.back()->SetBad();
    }
    std::vector<KeyFrame *> kfs;
    std::vector<std::vector<int>> neigh(n);
    for (int k = 0; k < n; k++) {
        int m, nn;
        if (fscanf(fp, "%d", &m) != 1) return fail("bad keyframe");
        KeyFrame *kf = new KeyFrame(1000 + k, maps[m], 0, 0, 0, 0, 0, nullptr);
        if (!read_bow(fp, kf->mBowVec) || fscanf(fp, "%d", &nn) != 1) return fail("bad keyframe vector");
        neigh[k].resize(nn);
        for (int j = 0; j < nn; j++) if (fscanf(fp, "%d", &neigh[k][j]) != 1) return fail("bad neighbour");
        kfs.push_back(kf);
    }
    for (int k = 0; k < n; k++) for (int j : neigh[k]) kfs[k]->mvpOrderedConnectedKeyFrames.push_back(kfs[j]);
    ORBVocabulary voc(1u << 20);
    KeyFrameDatabase::snSlots = n_slots > 0 ? n_slots : 1;
    KeyFrameDatabase::snMaxWords = 256;
    KeyFrameDatabase db(voc);
    if (feed)
        db.SetScoreFeed([&](const orbhip_kfdb_query &, int32_t *counts, std::vector<orbhip_kfdb_entry> &list) {
            if (fscanf(feed, "%d %d %d %d", &counts[0], &counts[1], &counts[2], &counts[3]) != 4) return false;
            for (int i = 0; i < counts[0] + counts[3]; i++) {
                int k, w, sc; unsigned b;
                if (fscanf(feed, "%d %d %d %u", &k, &w, &sc, &b) != 4 || i >= (int)list.size()) return false;
                list[i].slot = db.SlotOf(kfs[k]); list[i].words = w; list[i].scored = sc; list[i].score = float_of(b);
            }
            return true;
        });
    int nops;
    if (fscanf(fp, "%d", &nops) != 1) return fail("bad op count");
    std::atomic<bool> stop{false}; std::atomic<long> busy_calls{0}; std::atomic<int> busy_wrong{0};
    std::thread busy;
    if (threaded && !feed) busy = std::thread(busy_on_own_context, std::ref(stop), std::ref(busy_calls), std::ref(busy_wrong));
    std::vector<int> index_of;
    auto idx = [&](KeyFrame *p) { return (int)(std::find(kfs.begin(), kfs.end(), p) - kfs.begin()); };
    for (int i = 0; i < nops; i++) {
        char op[32];
        if (fscanf(fp, "%31s", op) != 1) return fail("bad op");
        std::vector<KeyFrame *> loop, merge, reloc;
        const std::string o(op);
        int a = 0;
        if (o == "add" || o == "erase" || o == "clear_map") { if (fscanf(fp, "%d", &a) != 1) return fail("bad operand"); }
        long unsigned int id = 0; int m = 0, ncand = 0, nconn = 0;
        DBoW2::BowVector bow;
        std::vector<int> conn;
        if (o == "nbest" || o == "reloc") {
            if (fscanf(fp, "%lu %d %d", &id, &m, &ncand) != 3 || !read_bow(fp, bow) || fscanf(fp, "%d", &nconn) != 1) return fail("bad query");
            conn.resize(nconn);
            for (int j = 0; j < nconn; j++) if (fscanf(fp, "%d", &conn[j]) != 1) return fail("bad connected list");
        } else if (o != "add" && o != "erase" && o != "clear_map" && o != "clear") return fail("unknown op");
        auto call = [&]() {
            if (o == "add") db.add(kfs[a]);
            else if (o == "erase") db.erase(kfs[a]);
            else if (o == "clear_map") db.clearMap(maps[a]);
            else if (o == "clear") db.clear();
            else if (o == "nbest") {
                KeyFrame q(id, maps[m], 0, 0, 0, 0, 0, nullptr);
                q.mBowVec = bow;
                for (int j : conn) q.mConnectedKeyFrameWeights[kfs[j]] = 1;
                db.DetectNBestCandidates(&q, loop, merge, ncand);
            } else {
                Frame F;
                F.mnId = id; F.mBowVec = bow;
                reloc = db.DetectRelocalizationCandidates(&F, maps[m]);
            }
        };
        if (threaded && i % 2 == 0) { std::thread th(call); th.join(); }      // a caller thread that is gone before the next call
        else call();
        printf("op %d\nloop", i);
        for (KeyFrame *p : loop) printf(" %d", idx(p));
        printf("\nmerge");
        for (KeyFrame *p : merge) printf(" %d", idx(p));
        printf("\nreloc");
        for (KeyFrame *p : reloc) printf(" %d", idx(p));
        printf("\n");
        for (int k = 0; k < n_slots; k++)
            printf("%d %lu %d %u %lu %d %u\n", k, kfs[k]->mnPlaceRecognitionQuery, kfs[k]->mnPlaceRecognitionWords, bits_of(kfs[k]->mPlaceRecognitionScore),
                   kfs[k]->mnRelocQuery, kfs[k]->mnRelocWords, bits_of(kfs[k]->mRelocScore));
    }
    fclose(fp);
    if (feed) fclose(feed);
    if (busy.joinable()) {
        stop = true; busy.join();
        fprintf(stderr, "busy thread: %ld calls on its own context, %s\n", busy_calls.load(), busy_wrong.load() ? "WRONG answers" : "all answers right");
        if (busy_wrong.load() || busy_calls.load() == 0) return 3;
    }
    return 0;
}

struct Lcg { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };

void random_bow(Lcg &r, int words, int vocab, DBoW2::BowVector &bow)
{
    while ((int)bow.size() < words) bow[r.next() % (uint32_t)vocab] = 1.0 + (r.next() % 1000) / 1000.0;
    double sum = 0;
    for (auto &e : bow) sum += e.second;
    for (auto &e : bow) e.second /= sum;
}

int latency(int nkf, int words, int vocab, int reps)
{
    Lcg r{12345};
    Map map0, map1;
    std::vector<KeyFrame *> kfs;
    for (int k = 0; k < nkf; k++) {
        KeyFrame *kf = new KeyFrame(k, (k % 4 == 3) ? &map1 : &map0, 0, 0, 0, 0, 0, nullptr);
        random_bow(r, words, vocab, kf->mBowVec);
        kfs.push_back(kf);
    }
    for (int k = 0; k < nkf; k++) for (int j = 1; j <= 10 && k - j >= 0; j++) kfs[k]->mvpOrderedConnectedKeyFrames.push_back(kfs[k - j]);
    ORBVocabulary voc((unsigned)vocab);
    KeyFrameDatabase::snSlots = nkf; KeyFrameDatabase::snMaxWords = words;
    KeyFrameDatabase db(voc);
    const auto t_add = std::chrono::steady_clock::now();
    for (KeyFrame *kf : kfs) db.add(kf);
    const double add_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_add).count();
    std::vector<double> nb, nb_dev, nb_tail, rl;
    size_t found = 0;
    for (int i = 0; i < reps + 3; i++) {                     // 3 warm-up calls
        KeyFrame q(100000 + i, &map0, 0, 0, 0, 0, 0, nullptr);
        q.mBowVec = kfs[(i * 37) % nkf]->mBowVec;             // a revisit of a stored place
        std::vector<KeyFrame *> loop, merge;
        auto t0 = std::chrono::steady_clock::now();
        db.DetectNBestCandidates(&q, loop, merge, 3);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const double dev_ms = db.mLastScoreCallMs, tail_ms = db.mLastTailMs;
        Frame F;
        F.mnId = 200000 + i; F.mBowVec = q.mBowVec;
        t0 = std::chrono::steady_clock::now();
        std::vector<KeyFrame *> rc = db.DetectRelocalizationCandidates(&F, &map0);
        const double ms2 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        found += loop.size() + merge.size() + rc.size();
        if (i >= 3) { nb.push_back(ms); nb_dev.push_back(dev_ms); nb_tail.push_back(tail_ms); rl.push_back(ms2); }
    }
    auto stat = [](std::vector<double> v, const char *name) {
        std::sort(v.begin(), v.end());
        printf("\"%s\": {\"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f}", name, v[v.size() / 2], v.front(), v.back());
    };
    printf("{\"keyframes\": %d, \"words\": %d, \"vocabulary\": %d, \"reps\": %d, \"candidates_found\": %zu, \"add_all_ms\": %.2f, ", nkf, words, vocab, reps, found, add_ms);
    stat(nb, "DetectNBestCandidates"); printf(", ");
    stat(rl, "DetectRelocalizationCandidates"); printf(", ");
    stat(nb_dev, "nbest_device_call"); printf(", ");
    stat(nb_tail, "nbest_host_tail"); printf("}\n");
    return found ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "run")) return run_script(argv[2], nullptr);
    if (argc >= 4 && !strcmp(argv[1], "tail")) return run_script(argv[2], argv[3]);
    if (argc >= 3 && !strcmp(argv[1], "threads")) return run_script(argv[2], argc > 3 ? argv[3] : nullptr, true);
    if (argc >= 2 && !strcmp(argv[1], "latency"))
        return latency(argc > 2 ? atoi(argv[2]) : 4096, argc > 3 ? atoi(argv[3]) : 1000, argc > 4 ? atoi(argv[4]) : 20000, argc > 5 ? atoi(argv[5]) : 20);
    fprintf(stderr, "usage: host_kfdb_smoke run SCRIPT | tail SCRIPT FEED | threads SCRIPT [FEED] | latency [KEYFRAMES WORDS VOCABULARY REPS]\n");
    return 2;
}
