/* Prints the size of isdqn_batch_conservative and the offsets of its members as the C compiler lays them out
 * (tests/test_conservative_host.py holds slimdqn._hip.BatchConservative to them).  Host C against include/isdqn_hip.h alone. */
#include <stddef.h>
#include <stdio.h>

#include "isdqn_hip.h"

int main(void) {
    printf("sizeof %zu\n", sizeof(isdqn_batch_conservative));
    printf("sizeof_batch %zu\n", sizeof(isdqn_batch));
    printf("sizeof_decay %zu\n", sizeof(isdqn_batch_decay));
    printf("flags %zu\n", offsetof(isdqn_batch_conservative, base.base.batch.flags));
    printf("loss_weights %zu\n", offsetof(isdqn_batch_conservative, base.base.batch.loss_weights));
    printf("discount %zu\n", offsetof(isdqn_batch_conservative, base.base.discount));
    printf("weight_decay %zu\n", offsetof(isdqn_batch_conservative, base.weight_decay));
    printf("decay_kinds %zu\n", offsetof(isdqn_batch_conservative, base.decay_kinds));
    printf("cql_alpha %zu\n", offsetof(isdqn_batch_conservative, cql_alpha));
    printf("reserved %zu\n", offsetof(isdqn_batch_conservative, reserved));
    printf("ISDQN_BATCH_CONSERVATIVE %d\n", ISDQN_BATCH_CONSERVATIVE);
    printf("ISDQN_BATCH_WEIGHT_DECAY %d\n", ISDQN_BATCH_WEIGHT_DECAY);
    return 0;
}
