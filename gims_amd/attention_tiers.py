"""The per-layer tier table of ``attention_precision='auto'`` and its decision rule (GMatcher.default_config describes the policy).

Host arithmetic on NumPy arrays only: GMatcher owns the device accumulator and its read-back, and hands every finished read-back to
``AttentionTiers.fold`` as one int64 array [layers][heads + 1][4] -- per head (sum of the row maxima, rows, largest row maximum, rows whose
maximum exceeds 1/2), the maxima in fixed point; in the last row the bit patterns of max |Q|, |K|, |V| as stored and the flag of a redo."""
import numpy as np

from .hip import ATTN_STAT_SCALE

MODE_NAMES = ('bf16', 'f16', 'bf16x3')


class AttentionTiers:
    """One table per generation of the weight pack.  mode: per layer 0 bf16 operands, 1 IEEE half, 2 split-bf16 pairs; new weights run every
    layer at 2 until the first measurement is in (`calibrated`), after which a layer only ever moves UP.  `config` is the model's config dict
    itself: the thresholds are read when they are used."""

    def __init__(self, n_layers, n_heads, gen, config):
        # peak, peak_max, tail: per (layer, head) as last measured (peak_max: the largest so far); range: largest |Q|, |K|, |V| seen per layer;
        # redone / rare: batches in which the device redid the layer / a diffuse bf16 layer had a sharply peaked row; rare_last: whether a
        # read-back folded in since begin() had one; switched: layers moved up after the first measurement, in order; batches: per stream
        # lane the index of its current batch
        self.gen, self.config, self.n_heads = gen, config, n_heads
        self.mode, self.calibrated, self.switched, self.batches = [2] * n_layers, False, [], {}
        self.peak, self.peak_max, self.tail, self.range = (np.zeros((n_layers, c)) for c in (n_heads, n_heads, n_heads, 3))
        self.redone, self.rare, self.rare_last = np.zeros(n_layers, dtype=np.int64), np.zeros(n_layers, dtype=np.int64), False

    def begin(self):
        """Start of a consume call: `rare_last` speaks of the read-backs folded in from here on (a call that finds none leaves it False -- an
        unmeasured batch never inherits the verdict of an earlier one)."""
        self.rare_last = False

    def measured(self, lane, repeat):
        """Count a batch of `lane` and say whether it is measured (`attention_monitor_period`; every batch until the table is calibrated).
        forward()'s repeat of a batch IS that batch: it is measured if the batch was -- the device-side guards it runs with read the statistic."""
        n_b = self.batches[lane] = self.batches.get(lane, -1) + (0 if repeat else 1)
        return not (self.calibrated and n_b % max(1, int(self.config['attention_monitor_period'])) != 0)

    def fold(self, raw, repeat=False):
        """Fold one read-back into the table.  Returns the number of layers a SETTLED table moved up by.  repeat: the read-back belongs to
        forward()'s repeat of a batch that was counted already -- its outlier rows are the same rows and do not count towards
        `attention_auto_rare_batches` a second time."""
        cfg, H, moved = self.config, self.n_heads, 0
        host = raw[:, :H, :].astype(np.float64)
        cnt = host[:, :, 1]
        seen = cnt > 0
        mean = np.where(seen, host[:, :, 0] / np.maximum(cnt, 1.0) / ATTN_STAT_SCALE, 0.0)
        tail = np.where(seen, host[:, :, 3] / np.maximum(cnt, 1.0), 0.0)
        rng = raw[:, H, :3].astype(np.uint32).view(np.float32).astype(np.float64)       # max |Q|, |K|, |V| as stored
        self.peak = np.where(seen, mean, self.peak)
        self.tail = np.where(seen, tail, self.tail)
        self.peak_max = np.maximum(self.peak_max, np.where(seen, host[:, :, 2] / ATTN_STAT_SCALE, 0.0))
        self.range = np.maximum(self.range, np.where(np.isfinite(rng), rng, np.inf))
        self.redone += (raw[:, H, 3] != 0)          # layers the device redid at split-bf16 inside that batch (guarded launches)
        hot = (mean > float(cfg['attention_auto_threshold'])).any(axis=1) | (tail > float(cfg['attention_auto_tail'])).any(axis=1)
        # a single sharply peaked row inside a diffuse bf16 layer: redone on the device by the guard (match_pairs), a reason for forward() to
        # repeat the batch with the guards on -- never a reason to move the layer up
        rmx = float(cfg['attention_auto_rowmax'])
        rare = (~hot) & (np.asarray(self.mode) == 0) & ((host[:, :, 2] / ATTN_STAT_SCALE >= rmx).any(axis=1) if rmx > 0 else False)
        self.rare = self.rare + (0 if repeat else rare)
        self.rare_last = self.rare_last or (bool(np.any(rare)) and self.calibrated)
        nb = int(cfg['attention_auto_rare_batches'])
        if nb > 0 and self.calibrated:          # no outlier any more: such a layer goes to the half tier like a sharpened one
            hot = hot | (rare & (self.rare >= nb))
        wide = (self.range > float(cfg['attention_f16_range'])).any(axis=1)
        want = np.where(hot, np.where(wide, 2, 1), 0)
        if not self.calibrated:
            if seen.all():
                self.mode = [int(w) for w in want]
                self.calibrated = True
        else:
            for l in np.nonzero(want > np.asarray(self.mode))[0]:
                self.mode[l] = int(want[l])
                self.switched.append(int(l))
                moved += 1
        return moved

    def report(self):
        """What GMatcher.attention_report() returns."""
        return dict(modes=[MODE_NAMES[v] for v in self.mode], calibrated=self.calibrated, peak=self.peak.copy(), peak_max=self.peak_max.copy(),
                    tail=self.tail.copy(), range=self.range.copy(), switched=list(self.switched), redone=self.redone.copy(), rare=self.rare.copy(),
                    threshold=float(self.config['attention_auto_threshold']), tail_threshold=float(self.config['attention_auto_tail']))

    def rebind(self, gen):
        """Carry the (settled) table over to the weight pack of generation `gen` (GMatcher._keep_attention_tiers, a test hook)."""
        self.gen = gen
