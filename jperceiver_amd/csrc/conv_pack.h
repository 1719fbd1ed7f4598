// Weight packing of the conv2d dispatchers (conv_pack.hip): the pack modes and the two functions through which the dispatchers
// (conv_fwd.hip, conv_dgrad.hip, conv_wgrad.hip; pack_p9 of conv_launch.h) issue a pack.  The recorder behind them
// (jp_pack_record_begin / _end) and the one-launch replay (jp_pack_replay) are ABI entry points of conv_pack.hip; these two are
// internal (hidden visibility).
#pragma once
#include "jp_common.h"

enum { PACK_TAP = 0, PACK_ROWMAJOR = 1, PACK_SEG = 2, PACK_UP_DGRAD = 3, PACK_FLIP = 4, PACK_FRAG = 5, PACK_FRAGSEG = 6, PACK_SPLIT = 7, PACK_SPLITSEG = 8, PACK_SPLITUPD = 9, PACK_SPLIT7 = 10 };

#pragma GCC visibility push(hidden)
// launches the pack now and, while a recording is open on this thread, appends its job descriptor to the caller's buffer
void do_pack(int mode, const float* w, float* wp, long total, int p0, int p1, int p2, int p3, int p4, int p5, hipStream_t st);
// tap-major pack wp[tap][row][Cp]: forward rows = co (src W[co][ci][tap]); dgrad rows = ci, reduction = co
void pack_weights(const float* w, float* wp, int Cout, int Cin, int KHW, int Cp, int for_dgrad, hipStream_t st);
#pragma GCC visibility pop
