/* Prints the size of isdqn_batch_mixture and the offsets of its members as the C compiler lays them out
 * (tests/test_mixture_host.py holds slimdqn._hip.BatchMixture to them).  Host C against include/isdqn_hip.h alone. */
#include <stddef.h>
#include <stdio.h>

#include "isdqn_hip.h"

int main(void) {
    printf("sizeof %zu\n", sizeof(isdqn_batch_mixture));
    printf("sizeof_conservative %zu\n", sizeof(isdqn_batch_conservative));
    printf("flags %zu\n", offsetof(isdqn_batch_mixture, base.base.base.batch.flags));
    printf("discount %zu\n", offsetof(isdqn_batch_mixture, base.base.base.discount));
    printf("weight_decay %zu\n", offsetof(isdqn_batch_mixture, base.base.weight_decay));
    printf("cql_alpha %zu\n", offsetof(isdqn_batch_mixture, base.cql_alpha));
    printf("alpha %zu\n", offsetof(isdqn_batch_mixture, alpha));
    printf("n_mix %zu\n", offsetof(isdqn_batch_mixture, n_mix));
    printf("reserved2 %zu\n", offsetof(isdqn_batch_mixture, reserved));
    printf("ISDQN_BATCH_MIXTURE %d\n", ISDQN_BATCH_MIXTURE);
    printf("ISDQN_ACT_MEAN_HEADS %d\n", ISDQN_ACT_MEAN_HEADS);
    return 0;
}
