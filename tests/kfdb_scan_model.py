"""A second statement of KeyFrameDatabase's two Detect... functions, in the formulation the device uses and sharing no code with
kfdb_model.py: no inverted file and no keyframe objects, only arrays indexed by slot.  The sharing list is the alive slots that share a
word with the query, ascending by (smallest shared word id, add sequence number); the state rules are applied per slot from the shared
count alone.  tests/test_kfdb_model.py shows the two agree on random scripts: that is the premise of scanning without linked lists."""
import numpy as np

PLACE, RELOC = 0, 1


class ScanDatabase:
    def __init__(self, capacity):
        self.capacity = capacity
        self.words = [np.zeros(0, np.int64) for _ in range(capacity)]
        self.values = [np.zeros(0, np.float64) for _ in range(capacity)]
        self.alive = np.zeros(capacity, bool)
        self.seq = np.zeros(capacity, np.int64)
        self.map = np.zeros(capacity, np.int64)
        self.query = np.zeros((capacity, 2), np.uint64)
        self.nwords = np.zeros((capacity, 2), np.int64)
        self.score = np.zeros((capacity, 2), np.float32)
        self.next_seq = 0

    def add(self, slot, map_id, words, values):
        assert not self.alive[slot]
        order = np.argsort(np.asarray(words, np.int64), kind="stable")
        self.words[slot] = np.asarray(words, np.int64)[order]
        self.values[slot] = np.asarray(values, np.float64)[order]
        self.alive[slot] = True; self.seq[slot] = self.next_seq; self.map[slot] = map_id
        self.next_seq += 1

    def erase(self, slot):
        self.alive[slot] = False

    def clear_map(self, map_id):
        self.alive &= self.map != map_id

    def clear(self):
        self.alive[:] = False
        self.query[:] = 0; self.nwords[:] = 0; self.score[:] = 0
        self.next_seq = 0

    def reset_slot(self, slot):
        self.query[slot] = 0; self.nwords[slot] = 0; self.score[slot] = 0

    def detect(self, qid, qmap, mode, words, values, connected=(), neighbours=None, n_candidates=3, bad_maps=()):
        """-> dict(sharing [(slot, words, scored, score)], touched [(slot, words)], max_common, scored [(slot, score, acc, best)],
        loop, merge, reloc).  neighbours: slot -> list of slots (-1: a keyframe without a slot)."""
        qw = np.asarray(words, np.int64); order = np.argsort(qw, kind="stable")
        qw = qw[order]; qv = np.asarray(values, np.float64)[order]
        conn = set(int(c) for c in connected if 0 <= int(c) < self.capacity) if mode == PLACE else set()
        listed, touched = [], []
        for s in np.nonzero(self.alive)[0]:
            common = np.intersect1d(self.words[s], qw, assume_unique=True)
            c = len(common)
            if c == 0:
                continue
            key = (int(common[0]), int(self.seq[s]), int(s))
            if self.query[s, mode] != np.uint64(qid):
                if int(s) in conn:
                    self.nwords[s, mode] = 1
                    touched.append(key)
                else:
                    self.query[s, mode] = np.uint64(qid); self.nwords[s, mode] = c
                    listed.append(key)
            else:
                self.nwords[s, mode] += c
                touched.append(key)
        listed.sort(); touched.sort()
        out = dict(sharing=[], touched=[(s, int(self.nwords[s, mode])) for _, _, s in touched], max_common=0, scored=[], loop=[], merge=[], reloc=[])
        if not listed:
            return out
        max_common = max(int(self.nwords[s, mode]) for _, _, s in listed)
        out["max_common"] = max_common
        min_common = int(np.float32(max_common) * np.float32(0.8))
        scored = []
        for _, _, s in listed:
            w = int(self.nwords[s, mode])
            if w > min_common:
                _, ia, ib = np.intersect1d(qw, self.words[s], assume_unique=True, return_indices=True)
                acc = np.float64(0)
                for a, b in zip(ia, ib):                                      # ascending shared word, one addition each
                    acc = acc + ((np.abs(qv[a] - self.values[s][b]) - np.abs(qv[a])) - np.abs(self.values[s][b]))
                si = np.float32(-acc / 2.0)
                self.score[s, mode] = si
                scored.append(s)
                out["sharing"].append((s, w, 1, si))
            else:
                out["sharing"].append((s, w, 0, np.float32(0)))
        if not scored or neighbours is None:
            return out
        best_acc = np.float32(0)
        for s in scored:
            si = self.score[s, mode]; best, acc, bs = si, si, s
            for nb in list(neighbours.get(s, []))[:10]:
                if nb < 0 or nb >= self.capacity or self.query[nb, mode] != np.uint64(qid):
                    continue
                acc = np.float32(acc + self.score[nb, mode])
                if self.score[nb, mode] > best:
                    bs, best = nb, self.score[nb, mode]
            out["scored"].append((s, si, acc, bs))
            if acc > best_acc:
                best_acc = acc
        bad = set(int(b) for b in bad_maps)
        if mode == RELOC:
            keep = np.float32(np.float32(0.75) * best_acc)
            for s, si, acc, bs in out["scored"]:
                if acc > keep and self.map[bs] == qmap and bs not in out["reloc"]:
                    out["reloc"].append(bs)
            return out
        rank = sorted(range(len(out["scored"])), key=lambda j: (-float(out["scored"][j][2]), j))
        seen = []
        for j in rank:
            bs = out["scored"][j][3]
            if bs in seen:
                continue
            seen.append(bs)
            if self.map[bs] == qmap:
                if len(out["loop"]) < n_candidates:
                    out["loop"].append(bs)
            elif int(self.map[bs]) not in bad and len(out["merge"]) < n_candidates:
                out["merge"].append(bs)
        return out
