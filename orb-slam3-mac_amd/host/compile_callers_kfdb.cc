// compile_callers_kfdb.cc -- compile-only check of the drop-in claim for KeyFrameDatabase: the reference's own call lines
// (src/LoopClosing.cc:278, :285, :292, :434, :463, :488; src/Tracking.cc:2634, :2819, :2883; src/KeyFrame.cc:744) against
// host/KeyFrameDatabase.h and the stand-ins of host/slam_types.h.  Nothing here runs.  Built by `make lib/compile_callers_kfdb.o` with
// -Wall -Werror, asserted by tests/test_kfdb_model.py.
#include <vector>
#include "KeyFrameDatabase.h"

using namespace std;

namespace ORB_SLAM3 {

struct LoopClosingKfdb {                  // the members of LoopClosing the lines mention
    KeyFrameDatabase *mpKeyFrameDB;
    KeyFrame *mpCurrentKF;
};

// LoopClosing::NewDetectCommonRegions: :278, :285, :292 (the early returns), :434, :463, :488
void loop_closing_lines(LoopClosingKfdb &S, vector<KeyFrame*> &vpLoopBowCand, vector<KeyFrame*> &vpMergeBowCand, int which)
{
    KeyFrameDatabase *mpKeyFrameDB = S.mpKeyFrameDB; KeyFrame *mpCurrentKF = S.mpCurrentKF;
    if (which == 0) {
        mpKeyFrameDB->add(mpCurrentKF);
        return;
    }
        // Search in BoW
        mpKeyFrameDB->DetectNBestCandidates(mpCurrentKF, vpLoopBowCand, vpMergeBowCand,3);

    mpKeyFrameDB->add(mpCurrentKF);
}

struct TrackingKfdb {                     // the members of Tracking the lines mention
    KeyFrameDatabase *mpKeyFrameDB;
    Frame mCurrentFrame;
    Atlas *mpAtlas;
};

// Tracking::Relocalization :2634, Tracking::Reset :2819, Tracking::ResetActiveMap :2883
bool tracking_lines(TrackingKfdb &S, Map *pMap, int which)
{
    KeyFrameDatabase *mpKeyFrameDB = S.mpKeyFrameDB; Frame &mCurrentFrame = S.mCurrentFrame; Atlas *mpAtlas = S.mpAtlas;
    if (which == 1) {
    mpKeyFrameDB->clear();
        return true;
    }
    if (which == 2) {
    mpKeyFrameDB->clearMap(pMap); // Only clear the active map references
        return true;
    }
    vector<KeyFrame*> vpCandidateKFs = mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame, mpAtlas->GetCurrentMap());

    if(vpCandidateKFs.empty()) {
        return false;
    }
    return true;
}

// KeyFrame::SetBadFlag :744 (`this` is the keyframe)
void keyframe_lines(KeyFrameDatabase *mpKeyFrameDB, KeyFrame *self)
{
    mpKeyFrameDB->erase(self);
}

// System::System (src/System.cc:159) constructs it from the vocabulary; LoopClosing / Tracking hand it on as a pointer
KeyFrameDatabase *system_lines(ORBVocabulary *mpVocabulary)
{
    KeyFrameDatabase *mpKeyFrameDatabase = new KeyFrameDatabase(*mpVocabulary);
    mpKeyFrameDatabase->SetORBVocabulary(mpVocabulary);
    return mpKeyFrameDatabase;
}

}  // namespace ORB_SLAM3
