"""CPU reference of the averaged readout traces (dpemu_feedline_traces,
include/dpemu.h; DESIGN.md §2 "Averaged traces and matched filter"): a plain
numpy restatement of the header comment on tests/feedline_ref.py's helpers
(the kept readouts and the state draw are dpemu_demod_feedline's).  Not test
code of its own: tests/test_traces.py validates the specification with it on
the CPU, tests/test_gpu_traces.py holds the kernel to it bit for bit.

``pairs`` is demod_iq_ref.demod_iq's dict of columns; ``lines`` a sequence of
sequences of pair indices.  Products and sums are int64: a product is at most
2^31 in magnitude and the entry point's bound keeps every sum below 2^62."""

import numpy as np

from tests.demod_iq_ref import s16
from tests.feedline_ref import _views, kept_readouts, state

TRACE_WORDS = 4
BINS_MAX = 4096


def check_bound(n_pairs, meas_cap, bin_clocks):
    """the bound the entry point refuses beyond (every sum then stays below 2^62)"""
    return n_pairs * meas_cap * bin_clocks * 16 <= 2 ** 31


def feedline_traces(cfg, pairs, lines, summary, events, adc, iq_lo, meas_cap, n_bins, bin_clocks=1, by_slot=False,
                    event_cap=None):
    """traces int64 (S, C, 2, n_bins, 4), S = meas_cap if by_slot else 1"""
    summary, events, event_cap = _views(summary, events, event_cap)
    adc = np.asarray(adc).view(np.uint32)
    iq_lo = np.asarray(iq_lo).view(np.uint32)
    n_pairs, n_lo = len(pairs['lane']), iq_lo.shape[1]
    assert 1 <= n_bins <= BINS_MAX and bin_clocks >= 1 and check_bound(n_pairs, meas_cap, bin_clocks)
    line_of = {p: l for l, line in enumerate(lines) for p in line}
    assert len(line_of) == n_pairs == sum(len(line) for line in lines)
    C_ = cfg.cores_per_shot
    out = np.zeros((meas_cap if by_slot else 1, C_, 2, n_bins, TRACE_WORDS), np.int64)
    for i in range(n_pairs):
        lane, core, shot = int(pairs['lane'][i]), int(pairs['core'][i]), int(pairs['shot'][i])
        spc_l = int(pairs['spc_lo'][i])
        lo, a = iq_lo[int(pairs['lo_row'][i])], adc[line_of[i]]
        for m, (t_lo, pe) in enumerate(kept_readouts(cfg, summary, events, lane, meas_cap, event_cap)):
            words = (pe >> 12) & 0xFFF or 4096
            j = np.arange(min(t_lo * spc_l, n_lo), min((t_lo + words * cfg.ro_cpw) * spc_l, n_lo), dtype=np.int64)
            a_i, a_q = s16(a[j]), s16(a[j] >> 16)
            lo_i, lo_q = s16(lo[j]), s16(lo[j] >> 16)
            p_i, p_q = a_i * lo_i + a_q * lo_q, a_q * lo_i - a_i * lo_q
            b = (j // spc_l - t_lo) // bin_clocks
            keep = b < n_bins
            row = out[m if by_slot else 0, core, state(cfg, shot, core, m)]
            np.add.at(row[:, 1], b[keep], 1)
            np.add.at(row[:, 2], b[keep], p_i[keep])
            np.add.at(row[:, 3], b[keep], p_q[keep])
            row[np.unique(b[keep]), 0] += 1
    return out
