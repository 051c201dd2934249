"""Diagnostic: per-phase cycle split of ctcx_beam_decode (s_memtime stamps).

Needs the counters build (the product library compiles them out):
  make -C ctc-beam-search-op_amd/csrc phases
  CTCEXT_LIB_PATH=$PWD/tools/libctcext_phases.so python tools/diag_phases.py B T W P [C]
(add -DCTCX_FASTLOOP_PROF to the phases build for the per-event split; that
build alone times make_heap, in counter 23).

Counter 14 is wave 0's wait for the frame's first chunk (a part of the queue
wait, counter 19), printed once.  In the small-C scored kernels the gather
counters 16..18 are the helper's first chunk in three spans.

CTCX_DIAG_LATE=1, with a phases build that adds -DCTCX_PHASE_LATE
(tools/build_variant.sh name "-DCTCX_PHASE_LATE" phases): the scored queue's
later chunks by chunk index -- wave 0's asks, how often and for how long the
chunk was late, the helper's scan steps or window passes spent on it.
CTCX_DIAG_BRANCH=0 names counter 31 for a -DCTCX_SPARSE_BRANCH=0 build."""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ctc-beam-search-op_amd"))
import numpy as np
import torch
import ctcext_amd
from ctcext_amd import _lib
B, T, W, P, C = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 29
x = torch.as_tensor(np.random.default_rng(20251015).standard_normal((T, B, C), dtype=np.float32), device="cuda")
sl = torch.full((B,), T, dtype=torch.int32, device="cuda")
f = _lib.CTCEXT_FLAG_PHASES | _lib.CTCEXT_FLAG_PROFILE
ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, flags=f)
out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, flags=f)
d = ctcext_amd.get_decoder(0)
NPH = 32   # ctcx_kernels.h kPhaseN: [0, 24) wave 0, [24, 32) the helper wave
LATE = bool(os.environ.get("CTCX_DIAG_LATE"))   # (a build with -DCTCX_PHASE_LATE: 64 more, by chunk index)
if LATE:
    NPH = 96
# the small-C helper's later chunks: filtered a branch per lane (the default
# build, CTCX_SPARSE_BRANCH=1: counter 31 counts window passes, plus the first
# chunk's one scan step) or an offer per lane (CTCX_DIAG_BRANCH=0 for a build
# with -DCTCX_SPARSE_BRANCH=0: scan steps)
BRANCH = os.environ.get("CTCX_DIAG_BRANCH", "1") != "0"
buf = np.zeros((B, NPH), np.uint64)
rc = d.lib.ctcext_phase_counters(d.handle, ctypes.c_void_p(buf.ctypes.data), B * NPH)
if rc != 0:
    sys.exit("ctcext_phase_counters failed (%d): %s" % (rc, d.lib.ctcext_last_error().decode()))
# the extract's std::sort frames (a beam no push changed, or one not full yet):
# their count rides in the upper half of counter 7, their cycles in counter 11's
sort_fr = (buf[:, 7] >> np.uint64(32)).astype(np.float64)
sort_cy = (buf[:, 11] >> np.uint64(32)).astype(np.float64)
buf[:, 7] &= np.uint64(0xFFFFFFFF)
buf[:, 11] &= np.uint64(0xFFFFFFFF)
m = buf.astype(np.float64).mean(0)
fr = m[7]
names = ["rowload", "recursion", "grow", "extract", "commit", "literal", "heap events", "frames",
         "scoring", "eventloop", "score:pre-skip", "chunks", "asm calls", "asm loop", "first-chunk wait", "flush",
         "gather (C>64)", "gather: window steps | C<=64: child-walk steps", "gather: windows | C<=64: child walk",
         "gather: top set",
         "gather: branch select", "gather: branches", "gather: S branches", "gather: select+S test+S hot"]
CYC = {0, 1, 2, 3, 4, 5, 8, 9, 10, 13, 14, 15, 16, 18, 19, 20, 23}
print("B=%d T=%d W=%d P=%d C=%d decode_ms=%.1f" % (B, T, W, P, C, d.last_stats["decode_kernel_ms"]))
sq_small = C <= 64 and m[30] > 0   # the small-C scored helper ran: 16..18 are its first-chunk spans
if os.environ.get("CTCX_DIAG_FASTLOOP"):   # (a build with -DCTCX_FASTLOOP_PROF)
    names[23] = "makeheap"
for k in range(24):
    if k == 7 or (sq_small and k in (16, 17, 18)):
        continue
    print("  %-10s %12.0f %s/frame" % (names[k], m[k] / fr, "cycles" if k in CYC else "count"))
if m[6] > 0:
    print("  asm loop cycles per push (incl. entry/exit): %.0f" % (m[13] / m[6]))
# per item: the kernel ends with its slowest item (one wave per item)
tot = buf[:, [0, 1, 2, 3, 4, 5]].astype(np.float64).sum(1)
o = np.argsort(tot)
print("  per-item cycles/frame: min %.0f mean %.0f max %.0f (items %s slowest)" % (
    tot.min() / fr, tot.mean() / fr, tot.max() / fr, list(o[-4:][::-1])))
for b in o[-3:][::-1]:
    print("    item %d: heap events %.0f/frame, extract %.0f, grow %.0f, eventloop %.0f, scoring %.0f" % (
        b, buf[b, 6] / fr, buf[b, 3] / fr, buf[b, 2] / fr, buf[b, 9] / fr, buf[b, 8] / fr))
print("  mean heap events/frame %.1f, max %.1f" % (buf[:, 6].mean() / fr, buf[:, 6].max() / fr))
# Extract() = std::sort: how many frames per item, what one costs, and what
# is left of the extract phase per sort_heap pop (W pops in every other frame)
if sort_fr.sum() > 0:
    ext = buf[:, 3].astype(np.float64)
    pops = (buf[:, 7].astype(np.float64) - sort_fr) * W
    print("  std::sort frames per item: mean %.1f min %.0f max %.0f of %.0f; %.0f cycles per sort (mean),"
          " %.0f cycles/frame over all frames, %.1f%% of the extract phase"
          % (sort_fr.mean(), sort_fr.min(), sort_fr.max(), fr, sort_cy.sum() / sort_fr.sum(),
             sort_cy.mean() / fr, 100.0 * sort_cy.sum() / max(1.0, ext.sum())))
    print("  extract without the sorts: %.0f cycles/frame, %.1f per sort_heap pop"
          % ((ext - sort_cy).mean() / fr, (ext - sort_cy).sum() / max(1.0, pops.sum())))
    items = list(o[-3:][::-1]) + [int(v) for v in os.environ.get("CTCX_DIAG_ITEMS", "").split(",") if v and int(v) < B]
    for b in items:
        print("    item %d: %.0f sort frames, %.0f cycles per sort, %.0f sort cycles/frame (mean item %.0f);"
              " all phases %.0f cycles/frame (mean item %.0f)"
              % (b, sort_fr[b], sort_cy[b] / max(1.0, sort_fr[b]), sort_cy[b] / fr, sort_cy.mean() / fr,
                 tot[b] / fr, tot.mean() / fr))
# two-wave kernels (cfg2/cfg3 class): the score-table wait and where the waves ran
if True:
    print("  HW table / queue wait %.0f cycles/frame, %.2f s_sleep rounds/frame (after the first chunk: %.0f cycles)"
          % (m[19] / fr, m[20] / fr, (m[19] - m[14]) / fr))
    w0, w1 = buf[:, 21].astype(np.int64), buf[:, 22].astype(np.int64)
    simd0, simd1 = (w0 >> 4) & 3, (w1 >> 4) & 3
    cu0, cu1 = (w0 >> 8) & 15, (w1 >> 8) & 15
    same_cu = (cu0 == cu1) & (((w0 >> 13) & 3) == ((w1 >> 13) & 3)) & (((w0 >> 12) & 1) == ((w1 >> 12) & 1))
    print("  HW waves: same CU %d/%d items, same SIMD %d/%d items (wave0 SIMD histogram %s, helper %s)" % (
        int(same_cu.sum()), B, int((same_cu & (simd0 == simd1)).sum()), B,
        np.bincount(simd0, minlength=4).tolist(), np.bincount(simd1, minlength=4).tolist()))
# the helper wave (two-wave scored-queue kernels; 0 where it does not run)
hn = {24: "helper gather (whole)", 25: "helper to first chunk", 26: "helper waits for wave 0",
      28: "helper rank extract", 29: "helper ring flush"}
for k, name in hn.items():
    print("  %-26s %10.0f cycles/frame" % (name, m[k] / fr))
step_name = "window passes (and the first chunk's scan step)" if (sq_small and BRANCH) else "scan steps"
print("  helper chunks %.2f/frame, %s %.2f/frame, child-walk steps %.2f/frame"
      % (m[30] / fr, step_name, m[31] / fr, m[27] / fr))
if m[31] > 0:
    busy = m[24] - m[26]
    print("  helper busy (gather minus waits for wave 0) %.0f cycles/frame, %.0f per %s" % (
        busy / fr, busy / m[31], "window pass or scan step" if (sq_small and BRANCH) else "scan step"))
if LATE:
    # wave 0's scored-chunk loop asks for chunk k (the kCtlReady test): how often, how
    # often the helper had not published it yet, and for how long wave 0 then slept
    print("  later chunks by index (the last row: every chunk from 15 on); cycles per frame over all frames")
    print("    chunk  asked/frame  late/frame  wait cycles/frame  wait per late ask  helper %s/frame"
          % ("passes" if BRANCH else "steps"))
    for k in range(16):
        ask, wait, steps, cnt = m[32 + k], m[48 + k], m[64 + k], m[80 + k]
        if ask == 0 and steps == 0:
            continue
        # (chunk 0 goes by the generic chunk path, which is not stamped: its wait is
        # the first-chunk wait above)
        print("    %5d  %11.3f  %10.3f  %17.0f  %17.0f  %14.2f" % (
            k, ask / fr, cnt / fr, wait / fr, wait / max(1.0, cnt), steps / fr))
    print("    all    %11.3f  %10.3f  %17.0f" % (m[32:48].sum() / fr, m[80:96].sum() / fr, m[48:64].sum() / fr))
if sq_small:
    print("  helper first chunk: entry to control words read %.0f, scan step %.0f, publish %.0f cycles/frame"
          % (m[16] / fr, m[17] / fr, m[18] / fr))
    # (counter 23 in these kernels: the helper's recursion of the next frame, CTCX_EARLY_RECURSE)
    print("  helper early recursion %.0f cycles/frame; early-recursed frames %d of %d"
          % (m[23] / fr, d.last_stats.get("early_recursed_frames", 0), B * T))
if os.environ.get("CTCX_DIAG_EXTP"):   # (a build with -DCTCX_PHASE_EXTP: the extract's stop)
    h = buf[:, 27].astype(np.uint64)
    cnt = [int(((h >> np.uint64(16 * k)) & np.uint64(0xFFFF)).sum()) for k in range(4)]
    nf = max(1, sum(cnt))
    print("  (raw helper words, items 0-3: %s)" % [hex(int(v)) for v in h[:4]])
    print("  extract stop (helper): p<=2 %.3f, 3..63 %.3f, 64..95 %.3f, 96..128 %.3f of %d frames" % (
        cnt[0] / nf, cnt[1] / nf, cnt[2] / nf, cnt[3] / nf, nf))
    print("  extract: wave 0's stop mean %.1f, frames with a helper stop %.3f, pops %.1f per frame" % (
        m[16] / fr, m[17] / fr, m[18] / fr))
if os.environ.get("CTCX_DIAG_TIES"):   # (a build with -DCTCX_PHASE_TIES: the first tied pair at rank p)
    nt = max(1.0, m[25])
    print("  ties (two new children, one label): %.3f of frames; parents: label = child's (sum of 2) %.3f,"
          " one the other's parent %.3f, siblings %.3f, same label %.3f, equal totals %.3f, blank = other's total %.3f"
          % (m[25] / fr, m[29] / nt, m[30] / nt, m[27] / nt, m[26] / nt, m[24] / nt, m[31] / nt))
if os.environ.get("CTCX_DIAG_EXTT"):   # (a build with -DCTCX_PHASE_EXTT: when the helper's stop lands)
    print("  extract: helper stop published in %.3f of frames, %.0f cycles after wave 0's extract start;"
          " asm segments %.2f per frame, %.1f pops, %.0f cycles in them (%.0f per pop), extract phase %.0f"
          % (m[26] / fr, m[25] / max(1.0, m[26]), m[17] / fr, m[18] / fr, m[23] / fr, m[23] / max(1.0, m[18]), m[3] / fr))
if os.environ.get("CTCX_DIAG_EXTT"):
    print("  helper: kCtlDone seen %.0f cycles after wave 0's extract start (all frames it ranks), rank to publish %.0f"
          % (m[24] / max(1.0, m[26]), m[27] / max(1.0, m[26])))
if os.environ.get("CTCX_DIAG_BIRTH"):   # (a build with -DCTCX_PHASE_BIRTH)
    print("  ties: frames ending without a tie %.3f; after such a frame, frames ending with one %.4f (of %.0f per item)"
          % (m[28] / fr, m[31] / max(1.0, m[30]), m[30]))

