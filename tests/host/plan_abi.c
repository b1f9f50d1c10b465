/* Plain C99 caller of emei_evaluate_sequences: include/emei_hip.h declares it in C, the library exports it.  Built (compiled and
 * linked, not run) by tests/test_plan_api.py with
 *   gcc -std=c99 -Wall -Werror -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ ... -lemei_hip -lamdhip64
 * Run, it checks the host-side argument validation, which touches no device. */
#include <stdint.h>
#include <stdio.h>

#include "emei_hip.h"

static int refused(int rc, const char* what) {
    if (rc != EMEI_ERR_INVALID) {
        printf("%s: expected EMEI_ERR_INVALID, got %d\n", what, rc);
        return 1;
    }
    if (emei_last_error()[0] == '\0') {
        printf("%s: no error text\n", what);
        return 1;
    }
    return 0;
}

int main(void) {
    uint8_t actions[4] = {0, 1, 0, 1};
    double ret[2];
    int32_t len[2];
    float final_obs[8];
    int bad = 0;
    if (emei_abi_version() != EMEI_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
    bad |= refused(emei_evaluate_sequences(NULL, 2, 2, actions, EMEI_ACT_U8, 1.0, NULL, ret, len, final_obs, NULL), "null handle");
    bad |= refused(emei_evaluate_sequences(NULL, 0, 2, actions, EMEI_ACT_U8, 1.0, NULL, ret, len, NULL, NULL), "horizon 0");
    bad |= refused(emei_evaluate_sequences(NULL, 2, 0, actions, EMEI_ACT_U8, 1.0, NULL, ret, len, NULL, NULL), "no candidates");
    bad |= refused(emei_evaluate_sequences(NULL, 2, 2, actions, EMEI_ACT_U8, 0.0, NULL, ret, len, NULL, NULL), "discount 0");
    bad |= refused(emei_evaluate_sequences(NULL, 2, 2, actions, EMEI_ACT_U8, 1.5, NULL, ret, len, NULL, NULL), "discount 1.5");
    if (bad) return 1;
    printf("PLAN ABI OK\n");
    return 0;
}
