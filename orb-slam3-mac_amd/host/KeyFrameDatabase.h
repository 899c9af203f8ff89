// KeyFrameDatabase.h -- signature-preserving mirror of the reference's KeyFrameDatabase (include/KeyFrameDatabase.h,
// src/KeyFrameDatabase.cc:35-98, :612-895) on the device-resident database of include/orbhip.h (orbhip_kfdb_*): same public members, same
// argument types, same results.  The inverted file is gone: every keyframe handed to add() gets a SLOT of one orbhip_kfdb on the object's
// own context and its mBowVec is uploaded there; a Detect... call makes ONE orbhip_kfdb_score_host call (the query's vector and, for
// DetectNBestCandidates, the slots of GetConnectedKeyFrames() up; the sharing list with words and scores down), writes
// mnPlaceRecognitionQuery / Words / Score (or the mnReloc... three) of every keyframe the reference would have touched, and then walks the
// covisibility accumulation and the selection on the host as the reference does -- tens of keyframes times ten neighbours, reading the
// fields just written.  DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no caller in the reference and are not
// mirrored; neither are PreSave / PostLoad.
// One deviation: the reference's `if(pKFi->isBad()) continue;` (src/KeyFrameDatabase.cc:735) does not advance its iterators and would
// never end; a bad keyframe has been erased from the database and from every covisibility list, so it cannot be reached -- here such
// an entry is passed over.
// Without a usable GPU: one message on stderr, empty results, no CPU fallback.
// Capacity: snSlots keyframes of at most snMaxWords words each (both read when the device database is created, at the first add or
// Detect... call).  A keyframe that was erased keeps its slot, and with it its state on the device, until the slots run out; then the
// slot erased longest ago is handed on, with its state reset.
// Threads: the reference calls one KeyFrameDatabase from LoopClosing (add, DetectNBestCandidates), Tracking
// (DetectRelocalizationCandidates, clear, clearMap) and whichever thread runs KeyFrame::SetBadFlag (erase).  The object therefore owns an
// orbhip_ctx of ITS OWN (own stream, own arenas) on hip::GetDevice(), created with the database at the first use, used only under the
// object's mutex and destroyed after the database in the destructor -- never a calling thread's hip::ThreadContext(), which that thread's
// matchers use at the same time and which dies with the thread.
#pragma once
#include <functional>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "../../include/orbhip.h"
#ifdef ORBHIP_WITH_ORBSLAM3
#include "ORBVocabulary.h"
#endif
#include "slam_types.h"

namespace ORB_SLAM3 {

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc);
    ~KeyFrameDatabase();

    void add(KeyFrame *pKF);
    void erase(KeyFrame *pKF);
    void clear();
    void clearMap(Map *pMap);

    // Loop, merge and relocalisation candidates
    void DetectNBestCandidates(KeyFrame *pKF, std::vector<KeyFrame *> &vpLoopCand, std::vector<KeyFrame *> &vpMergeCand, int nNumCandidates);
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F, Map *pMap);

    void SetORBVocabulary(ORBVocabulary *pORBVoc);

    static int snSlots;        // 4096
    static int snMaxWords;     // 2048 (<= 4096)

#ifdef ORBHIP_KFDB_TEST_HOOKS
    // test plumbing, compiled into lib/host_kfdb_smoke only: what stands in for the device call of a Detect... -- given the query record it
    // fills counts[4] and the list rows as orbhip_kfdb_score_host would; with a feed set nothing touches a device
    typedef std::function<bool(const orbhip_kfdb_query &, int32_t *, std::vector<orbhip_kfdb_entry> &)> ScoreFeed;
    void SetScoreFeed(ScoreFeed feed) { mFeed = feed; }
    int SlotOf(KeyFrame *pKF);                               // -1: never added
    double mLastScoreCallMs = 0, mLastTailMs = 0;            // wall time of the last Detect...'s device call and of its host tail
#endif

protected:
    bool Ready();                                            // the device database exists (or a feed stands in)
    int MapId(Map *pMap);
    int TakeSlot(KeyFrame *pKF, bool &recycled);
    // the device call and the state write-back; false: nothing usable came back.  vScored: the scored keyframes in list order
    bool Score(long unsigned int nId, Map *pMap, int mode, const DBoW2::BowVector &vBow, const std::set<KeyFrame *> *pConnected,
               std::vector<std::pair<float, KeyFrame *>> &vScored);

    const ORBVocabulary *mpVoc;
    orbhip_ctx *mpCtx;                                       // the object's own context (see "Threads" above)
    orbhip_kfdb *mpDB;
    bool mbTried;
    std::map<KeyFrame *, int> mSlot;                         // every keyframe that holds a slot, alive or erased
    std::vector<KeyFrame *> mvSlotKF;                        // slot -> keyframe (nullptr: free)
    std::vector<unsigned char> mvAlive;
    std::list<int> mlErased;                                 // erased slots, oldest first
    std::map<Map *, int> mMapId;
#ifdef ORBHIP_KFDB_TEST_HOOKS
    ScoreFeed mFeed;
#endif
    std::mutex mMutex;
};

}  // namespace ORB_SLAM3
