/* Prints the size of isdqn_batch_decay and the offsets of its members as the C compiler lays them out (tests/test_adamw_host.py holds
 * slimdqn._hip.BatchDecay to them).  Host C against include/isdqn_hip.h alone. */
#include <stddef.h>
#include <stdio.h>

#include "isdqn_hip.h"

int main(void) {
    printf("sizeof %zu\n", sizeof(isdqn_batch_decay));
    printf("sizeof_batch %zu\n", sizeof(isdqn_batch));
    printf("sizeof_discount %zu\n", sizeof(isdqn_batch_discount));
    printf("flags %zu\n", offsetof(isdqn_batch_decay, base.batch.flags));
    printf("loss_weights %zu\n", offsetof(isdqn_batch_decay, base.batch.loss_weights));
    printf("discount %zu\n", offsetof(isdqn_batch_decay, base.discount));
    printf("weight_decay %zu\n", offsetof(isdqn_batch_decay, weight_decay));
    printf("decay_kinds %zu\n", offsetof(isdqn_batch_decay, decay_kinds));
    printf("ISDQN_BATCH_WEIGHT_DECAY %d\n", ISDQN_BATCH_WEIGHT_DECAY);
    printf("ISDQN_DECAY_KINDS_KERNELS %d\n", ISDQN_DECAY_KINDS_KERNELS);
    printf("ISDQN_DECAY_KINDS_ALL %d\n", ISDQN_DECAY_KINDS_ALL);
    return 0;
}
