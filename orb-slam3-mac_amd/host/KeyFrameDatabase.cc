// KeyFrameDatabase.cc -- see KeyFrameDatabase.h
#include "KeyFrameDatabase.h"
#include <chrono>
#include <cstdio>
#include "hip_context.h"

#ifdef ORBHIP_KFDB_TEST_HOOKS
#define KFDB_FEED (mFeed)
#else
#define KFDB_FEED (false)
#endif

using namespace std;

namespace ORB_SLAM3 {

int KeyFrameDatabase::snSlots = 4096;
int KeyFrameDatabase::snMaxWords = 2048;

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc), mpCtx(nullptr), mpDB(nullptr), mbTried(false) {}

KeyFrameDatabase::~KeyFrameDatabase()
{
    if (mpDB) orbhip_kfdb_destroy(mpDB);                     // synchronises the context's stream first
    if (mpCtx) orbhip_ctx_destroy(mpCtx);
}

void KeyFrameDatabase::SetORBVocabulary(ORBVocabulary *pORBVoc) { mpVoc = pORBVoc; }

bool KeyFrameDatabase::Ready()
{
    if (mvSlotKF.empty()) { mvSlotKF.assign(snSlots > 0 ? snSlots : 1, nullptr); mvAlive.assign(mvSlotKF.size(), 0); }
    if (KFDB_FEED) return true;
    if (mpDB) return true;
    if (mbTried) return false;
    mbTried = true;
    // a context of the object's own, not the calling thread's: several threads call this object, each busy on its own context meanwhile
    int rc = orbhip_ctx_create(hip::GetDevice(), nullptr, &mpCtx);
    if (rc != ORBHIP_OK) {
        mpCtx = nullptr;
        fprintf(stderr, "KeyFrameDatabase: no device context on GPU %d: %d (%s) -- this build needs an MI355X, there is no CPU fallback\n", hip::GetDevice(), rc,
                orbhip_last_error());
        return false;
    }
    rc = orbhip_kfdb_create(mpCtx, (int)mvSlotKF.size(), snMaxWords, &mpDB);
    if (rc != ORBHIP_OK) {
        mpDB = nullptr;
        orbhip_ctx_destroy(mpCtx); mpCtx = nullptr;
        fprintf(stderr, "KeyFrameDatabase: no device database (%d: %s)\n", rc, orbhip_last_error());
        return false;
    }
    return true;
}

int KeyFrameDatabase::MapId(Map *pMap)
{
    auto it = mMapId.find(pMap);
    if (it != mMapId.end()) return it->second;
    const int id = (int)mMapId.size();
    mMapId[pMap] = id;
    return id;
}

#ifdef ORBHIP_KFDB_TEST_HOOKS
int KeyFrameDatabase::SlotOf(KeyFrame *pKF)                  // no lock: a feed calls it from inside a Detect...
{
    auto it = mSlot.find(pKF);
    return it == mSlot.end() ? -1 : it->second;
}
#endif

int KeyFrameDatabase::TakeSlot(KeyFrame *pKF, bool &recycled)
{
    recycled = false;
    auto it = mSlot.find(pKF);
    if (it != mSlot.end()) { mlErased.remove(it->second); return it->second; }
    if (mSlot.size() < mvSlotKF.size()) {                     // a slot is never given back, so the used ones are [0, mSlot.size())
        const int s = (int)mSlot.size();
        mvSlotKF[s] = pKF; mSlot[pKF] = s;
        return s;
    }
    if (mlErased.empty()) return -1;
    const int s = mlErased.front();
    mlErased.pop_front();
    mSlot.erase(mvSlotKF[s]);
    mvSlotKF[s] = pKF; mSlot[pKF] = s;
    recycled = true;
    return s;
}

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    unique_lock<mutex> lock(mMutex);
    if (!Ready()) return;
    bool recycled = false;
    const int slot = TakeSlot(pKF, recycled);
    if (slot < 0) { fprintf(stderr, "KeyFrameDatabase::add: all %d slots hold live keyframes; keyframe %lu is not added\n", (int)mvSlotKF.size(), pKF->mnId); return; }
    if (mvAlive[slot]) return;                               // added twice: the reference would list it twice; callers do not
    if (!KFDB_FEED) {
        vector<int32_t> w; vector<double> v;
        w.reserve(pKF->mBowVec.size()); v.reserve(pKF->mBowVec.size());
        for (const auto &e : pKF->mBowVec) { w.push_back((int32_t)e.first); v.push_back(e.second); }
        int rc = recycled ? orbhip_kfdb_reset_slot(mpDB, slot) : ORBHIP_OK;
        if (rc == ORBHIP_OK) rc = orbhip_kfdb_add_host(mpDB, slot, MapId(pKF->GetMap()), w.data(), v.data(), (int)w.size());
        if (rc != ORBHIP_OK) {
            fprintf(stderr, "KeyFrameDatabase::add: keyframe %lu not added (%d: %s)\n", pKF->mnId, rc, orbhip_last_error());
            mlErased.push_back(slot);
            return;
        }
    }
    mvAlive[slot] = 1;
}

void KeyFrameDatabase::erase(KeyFrame *pKF)
{
    unique_lock<mutex> lock(mMutex);
    auto it = mSlot.find(pKF);
    if (it == mSlot.end() || !mvAlive[it->second]) return;
    if (!KFDB_FEED && mpDB) orbhip_kfdb_erase(mpDB, it->second);
    mvAlive[it->second] = 0;
    mlErased.push_back(it->second);
}

void KeyFrameDatabase::clear()
{
    unique_lock<mutex> lock(mMutex);
    // the reference empties the inverted file and leaves the keyframes' fields alone: the slots are erased, not zeroed, so that a keyframe
    // added again meets its old state
    for (size_t s = 0; s < mvSlotKF.size(); s++)
        if (mvAlive[s]) {
            if (!KFDB_FEED && mpDB) orbhip_kfdb_erase(mpDB, (int)s);
            mvAlive[s] = 0;
            mlErased.push_back((int)s);
        }
}

void KeyFrameDatabase::clearMap(Map *pMap)
{
    unique_lock<mutex> lock(mMutex);
    if (!mMapId.count(pMap)) return;
    if (!KFDB_FEED && mpDB) orbhip_kfdb_clear_map(mpDB, mMapId[pMap]);
    for (size_t s = 0; s < mvSlotKF.size(); s++)
        if (mvAlive[s] && mvSlotKF[s]->GetMap() == pMap) { mvAlive[s] = 0; mlErased.push_back((int)s); }
}

bool KeyFrameDatabase::Score(long unsigned int nId, Map *pMap, int mode, const DBoW2::BowVector &vBow, const set<KeyFrame *> *pConnected,
                             vector<pair<float, KeyFrame *>> &vScored)
{
    if (!Ready()) return false;
    orbhip_kfdb_query q;
    q.id = nId; q.map_id = MapId(pMap); q.mode = mode;
    vector<int32_t> w, conn; vector<double> v;
    for (const auto &e : vBow) { w.push_back((int32_t)e.first); v.push_back(e.second); }
    if (pConnected)
        for (KeyFrame *pKFc : *pConnected) { auto it = mSlot.find(pKFc); if (it != mSlot.end()) conn.push_back(it->second); }
    const int max_list = (int)mvSlotKF.size() < ORBHIP_KFDB_MAX_LIST ? (int)mvSlotKF.size() : ORBHIP_KFDB_MAX_LIST;
    vector<orbhip_kfdb_entry> list(max_list);
    int32_t counts[4] = {0, 0, 0, 0};
#ifdef ORBHIP_KFDB_TEST_HOOKS
    const auto t0 = chrono::steady_clock::now();
    if (mFeed) {
        if (!mFeed(q, counts, list)) return false;
    } else
#endif
    {
        const int rc = orbhip_kfdb_score_host(mpDB, &q, w.data(), v.data(), (int)w.size(), conn.data(), (int)conn.size(), max_list, counts, list.data());
        if (rc != ORBHIP_OK) {
            fprintf(stderr, "KeyFrameDatabase: the device query failed (%d: %s); no candidates\n", rc, orbhip_last_error());
            return false;
        }
    }
#ifdef ORBHIP_KFDB_TEST_HOOKS
    mLastScoreCallMs = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
#endif
    // leave every keyframe's fields as the reference does: listed ones get the id, the words and, when scored, the score; the ones met
    // without being listed (connected keyframes, a repeated id) only their words
    for (int i = 0; i < counts[0] + counts[3]; i++) {
        KeyFrame *pKFi = mvSlotKF[list[i].slot];
        const bool listed = i < counts[0];
        if (mode == ORBHIP_KFDB_PLACE) {
            pKFi->mnPlaceRecognitionWords = list[i].words;
            if (listed) pKFi->mnPlaceRecognitionQuery = nId;
            if (listed && list[i].scored) pKFi->mPlaceRecognitionScore = list[i].score;
        } else {
            pKFi->mnRelocWords = list[i].words;
            if (listed) pKFi->mnRelocQuery = nId;
            if (listed && list[i].scored) pKFi->mRelocScore = list[i].score;
        }
        if (listed && list[i].scored) vScored.push_back(make_pair(list[i].score, pKFi));
    }
    return true;
}

namespace {
// one scored keyframe with its ten best covisible ones: the summed score and the keyframe of the group with the highest own score
template <class Marked, class ScoreOf>
pair<float, KeyFrame *> accumulate(const pair<float, KeyFrame *> &entry, Marked marked, ScoreOf score_of)
{
    float best = entry.first, acc = entry.first;
    KeyFrame *pBest = entry.second;
    for (KeyFrame *pKF2 : entry.second->GetBestCovisibilityKeyFrames(ORBHIP_KFDB_NEIGHBOURS)) {
        if (!marked(pKF2)) continue;
        const float s = score_of(pKF2);
        acc += s;
        if (s > best) { pBest = pKF2; best = s; }
    }
    return make_pair(acc, pBest);
}
}  // namespace

void KeyFrameDatabase::DetectNBestCandidates(KeyFrame *pKF, vector<KeyFrame *> &vpLoopCand, vector<KeyFrame *> &vpMergeCand, int nNumCandidates)
{
    unique_lock<mutex> lock(mMutex);
    const set<KeyFrame *> spConnectedKF = pKF->GetConnectedKeyFrames();
    vector<pair<float, KeyFrame *>> vScored;
    if (!Score(pKF->mnId, pKF->GetMap(), ORBHIP_KFDB_PLACE, pKF->mBowVec, &spConnectedKF, vScored) || vScored.empty()) return;
#ifdef ORBHIP_KFDB_TEST_HOOKS
    const auto t0 = chrono::steady_clock::now();
#endif
    const long unsigned int nId = pKF->mnId;
    list<pair<float, KeyFrame *>> lAcc;
    for (const auto &e : vScored)
        lAcc.push_back(accumulate(e, [nId](KeyFrame *k) { return k->mnPlaceRecognitionQuery == nId; }, [](KeyFrame *k) { return k->mPlaceRecognitionScore; }));
    lAcc.sort([](const pair<float, KeyFrame *> &a, const pair<float, KeyFrame *> &b) { return a.first > b.first; });       // stable: ties keep list order
    vpLoopCand.reserve(nNumCandidates);
    vpMergeCand.reserve(nNumCandidates);
    set<KeyFrame *> spSeen;
    for (auto it = lAcc.begin(); it != lAcc.end() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates); ++it) {
        KeyFrame *pKFi = it->second;
        if (pKFi->isBad()) continue;                          // the deviation: passed over (KeyFrameDatabase.h)
        if (!spSeen.insert(pKFi).second) continue;
        const bool same = pKF->GetMap() == pKFi->GetMap();
        if (same && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(pKFi);
        else if (!same && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);
    }
#ifdef ORBHIP_KFDB_TEST_HOOKS
    mLastTailMs = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
#endif
}

vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F, Map *pMap)
{
    unique_lock<mutex> lock(mMutex);
    vector<pair<float, KeyFrame *>> vScored;
    // the candidates must be of pMap, but every map's keyframes are met, counted and scored, as in the reference
    if (!Score(F->mnId, pMap, ORBHIP_KFDB_RELOC, F->mBowVec, nullptr, vScored) || vScored.empty()) return vector<KeyFrame *>();
#ifdef ORBHIP_KFDB_TEST_HOOKS
    const auto t0 = chrono::steady_clock::now();
#endif
    const long unsigned int nId = F->mnId;
    vector<pair<float, KeyFrame *>> vAcc;
    float bestAccScore = 0;
    for (const auto &e : vScored) {
        vAcc.push_back(accumulate(e, [nId](KeyFrame *k) { return k->mnRelocQuery == nId; }, [](KeyFrame *k) { return k->mRelocScore; }));
        if (vAcc.back().first > bestAccScore) bestAccScore = vAcc.back().first;
    }
    const float minScoreToRetain = 0.75f * bestAccScore;
    set<KeyFrame *> spSeen;
    vector<KeyFrame *> vpRelocCandidates;
    vpRelocCandidates.reserve(vAcc.size());
    for (const auto &a : vAcc)
        if (a.first > minScoreToRetain && a.second->GetMap() == pMap && spSeen.insert(a.second).second) vpRelocCandidates.push_back(a.second);
#ifdef ORBHIP_KFDB_TEST_HOOKS
    mLastTailMs = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
#endif
    return vpRelocCandidates;
}

}  // namespace ORB_SLAM3
