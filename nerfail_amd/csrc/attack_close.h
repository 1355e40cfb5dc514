// The epoch close of the attack loops, AS:405-431 and IG:392-416, as ONE device function: nerfail_attack_epoch_close
// (attack_stats.hip; a tie goes to the later epoch) and nerfail_u2d_epoch_close (u2d.hip; strict, a tie keeps the earlier epoch)
// differ in the comparison alone. Row, best and record layouts: include/nerfail_hip.h.
#pragma once
#include "common.h"

namespace nerfail {

__device__ __forceinline__ void attack_epoch_close_body(const float* __restrict__ row, float* __restrict__ best, int epoch, int targeted,
                                                        bool strict, float* __restrict__ record, int* __restrict__ flag) {
    const double views = (double)row[6];
    const float test_loss = (float)(pair_get(row + 0) / views), attack_loss = (float)(pair_get(row + 2) / views);
    const float test_acc = (float)((double)row[4] / views), attack_acc = (float)((double)row[5] / views);
    const float img_loss = (float)(pair_get(row + 7) / pair_get(row + 9));
    const float best_acc = best[0];
    bool take;                                                                              // false for a NaN accuracy
    if (strict) take = targeted ? (attack_acc > best_acc) : (attack_acc < best_acc);
    else take = targeted ? (attack_acc >= best_acc) : (attack_acc <= best_acc);
    if (take) {
        best[0] = attack_acc;
        best[1] = attack_loss;
        best[2] = (float)epoch;
    }
    flag[0] = take ? 1 : 0;
    record[0] = test_loss;
    record[1] = test_acc;
    record[2] = attack_loss;
    record[3] = attack_acc;
    record[4] = img_loss;
    record[5] = row[6];
    record[6] = take ? 1.f : 0.f;
    record[7] = take ? (float)epoch : best[2];
    record[8] = take ? attack_acc : best_acc;
    record[9] = take ? attack_loss : best[1];
    record[10] = (float)epoch;
    record[11] = row[4];
    record[12] = row[5];
    record[13] = record[14] = record[15] = 0.f;
}

}  // namespace nerfail
