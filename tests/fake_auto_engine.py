"""FakeEngine with the three calls distributed.sharded_assemble(auto_limit=True) needs -- TEST
INFRASTRUCTURE ONLY.  They restate ec_dense_spectrum / ec_dense_refilter / ec_export_dense on the
records the fake merge holds: a histogram of the counts with a saturating last bin, a filter
count > limit that keeps the order, and the records as they are."""
import numpy as np

from fake_engine import FakeEngine


class FakeAutoEngine(FakeEngine):
    def __init__(self, k):
        super().__init__(k)
        self.auto_calls = []  # the new calls, in order

    def dense_spectrum(self, nbins=1024):
        self.auto_calls.append(("dense_spectrum", int(nbins)))
        h = np.zeros(nbins, np.uint64)
        np.add.at(h, np.minimum(self.recs["count"].astype(np.int64), nbins - 1), 1)
        return h

    def dense_refilter(self, limit):
        self.auto_calls.append(("dense_refilter", int(limit)))
        keep = self.recs["count"] > limit
        removed = int((~keep).sum())
        if removed:
            self.recs = self.recs[keep].copy()
        return len(self.recs), {"limit": int(limit), "changed": int(removed > 0), "n_removed_kmers": removed}

    def export_dense(self):
        self.auto_calls.append(("export_dense",))
        return self._bytes(self.recs)
