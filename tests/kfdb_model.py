"""Plain-Python transcription of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc:35-98 add / erase / clear / clearMap, :612-780
DetectNBestCandidates, :783-895 DetectRelocalizationCandidates) and of L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68):
an inverted file of per-word lists, keyframe objects carrying the six state fields, numpy.float32 / float64 at the reference's roundings.
The yardstick of the device path and of host/KeyFrameDatabase.cc; written from the reference's text, not run against a DBoW2 build."""
import numpy as np

F32 = np.float32


class Map:
    def __init__(self, mid, bad=False):
        self.id, self.bad = mid, bad

    def IsBad(self):
        return self.bad


class KeyFrame:
    """the fields KeyFrameDatabase reads and writes; `slot` is the device slot (None: a keyframe the database never saw)"""
    def __init__(self, mnId, bow, pMap, slot=None):
        self.mnId = mnId
        self.mBowVec = dict(sorted((int(w), float(v)) for w, v in bow))       # std::map<WordId, WordValue>: ascending
        self.map = pMap
        self.slot = slot
        self.neighbours = []                                                  # mvpOrderedConnectedKeyFrames
        self.connected = set()                                                # GetConnectedKeyFrames()
        self.mnPlaceRecognitionQuery = 0; self.mnPlaceRecognitionWords = 0; self.mPlaceRecognitionScore = F32(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0; self.mRelocScore = F32(0)

    def GetMap(self):
        return self.map

    def GetBestCovisibilityKeyFrames(self, n):
        return self.neighbours[:n]

    def state(self):
        return (self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, F32(self.mPlaceRecognitionScore).tobytes(),
                self.mnRelocQuery, self.mnRelocWords, F32(self.mRelocScore).tobytes())

    def reset_state(self):
        self.mnPlaceRecognitionQuery = 0; self.mnPlaceRecognitionWords = 0; self.mPlaceRecognitionScore = F32(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0; self.mRelocScore = F32(0)


def l1_terms(v1, v2):
    """the terms L1Scoring::score adds, in its order (both maps ascending: the merge walk meets the shared words ascending)"""
    out = []
    for w in v1:                                                              # dict built sorted
        if w in v2:
            vi, wi = np.float64(v1[w]), np.float64(v2[w])
            out.append(np.float64(np.float64(abs(np.float64(vi - wi)) - abs(vi)) - abs(wi)))
    return out


def l1_score(v1, v2):
    score = np.float64(0)
    for t in l1_terms(v1, v2):
        score = np.float64(score + t)
    return np.float64(-score / np.float64(2.0))


class Result:
    """what one Detect... call did: sharing = lKFsSharingWords, scored = [(pKFi, si, accScore, pBestKF)] in list order, max_common,
    and the outputs"""
    def __init__(self):
        self.sharing, self.scored, self.max_common = [], [], 0
        self.loop, self.merge, self.reloc = [], [], []


class KeyFrameDatabase:
    def __init__(self):
        self.inv = {}                                                         # mvInvertedFile: word -> list<KeyFrame*>

    def add(self, pKF):
        for w in pKF.mBowVec:
            self.inv.setdefault(w, []).append(pKF)

    def erase(self, pKF):
        for w in pKF.mBowVec:
            lst = self.inv.get(w, [])
            for i, k in enumerate(lst):
                if k is pKF:
                    del lst[i]
                    break

    def clear(self):
        self.inv = {}

    def clearMap(self, pMap):
        for w in self.inv:
            self.inv[w] = [k for k in self.inv[w] if k.GetMap() is not pMap]

    def DetectNBestCandidates(self, pKF, nNumCandidates):
        r = Result()
        spConnectedKF = pKF.connected
        for w in pKF.mBowVec:
            for pKFi in self.inv.get(w, []):
                if pKFi.mnPlaceRecognitionQuery != pKF.mnId:
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi not in spConnectedKF:
                        pKFi.mnPlaceRecognitionQuery = pKF.mnId
                        r.sharing.append(pKFi)
                pKFi.mnPlaceRecognitionWords += 1
        if not r.sharing:
            return r
        maxCommonWords = 0
        for k in r.sharing:
            if k.mnPlaceRecognitionWords > maxCommonWords:
                maxCommonWords = k.mnPlaceRecognitionWords
        r.max_common = maxCommonWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in r.sharing:
            if pKFi.mnPlaceRecognitionWords > minCommonWords:
                si = F32(l1_score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mPlaceRecognitionScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return r
        lAcc = []
        for si, pKFi in lScoreAndMatch:
            bestScore = si; accScore = si; pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnPlaceRecognitionQuery != pKF.mnId:
                    continue
                accScore = F32(accScore + pKF2.mPlaceRecognitionScore)
                if pKF2.mPlaceRecognitionScore > bestScore:
                    pBestKF = pKF2; bestScore = pKF2.mPlaceRecognitionScore
            lAcc.append((accScore, pBestKF))
            r.scored.append((pKFi, si, accScore, pBestKF))
        lAcc.sort(key=lambda p: -float(p[0]))                                 # list::sort(compFirst): stable, descending
        seen = set()
        for acc, pKFi in lAcc:
            if not (len(r.loop) < nNumCandidates or len(r.merge) < nNumCandidates):
                break
            if id(pKFi) not in seen:
                if pKF.GetMap() is pKFi.GetMap() and len(r.loop) < nNumCandidates:
                    r.loop.append(pKFi)
                elif pKF.GetMap() is not pKFi.GetMap() and len(r.merge) < nNumCandidates and not pKFi.GetMap().IsBad():
                    r.merge.append(pKFi)
                seen.add(id(pKFi))
        return r

    def DetectRelocalizationCandidates(self, F, pMap):
        r = Result()
        for w in F.mBowVec:
            for pKFi in self.inv.get(w, []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    r.sharing.append(pKFi)
                pKFi.mnRelocWords += 1
        if not r.sharing:
            return r
        maxCommonWords = 0
        for k in r.sharing:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        r.max_common = maxCommonWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in r.sharing:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return r
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si; accScore = si; pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2; bestScore = pKF2.mRelocScore
            r.scored.append((pKFi, si, accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        seen = set()
        for pKFi, si, acc, pBest in r.scored:
            if acc > minScoreToRetain:
                if pBest.GetMap() is not pMap:
                    continue
                if id(pBest) not in seen:
                    r.reloc.append(pBest)
                    seen.add(id(pBest))
        return r
