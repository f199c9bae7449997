/* Prints the layout of the mag_buf boundary as one JSON object: offset and size of each of the eleven fields of
 * `struct mag_buf` (fifo.h:57-73), its sizeof and alignment, the flag and input-format values.
 *
 * Built two ways from this one file, and the two outputs must be equal:
 *   default                     the library's own declarations (modes_hip_readsb.h, struct msd_mag_buf)
 *   -DDUMP_REFERENCE -I<ref>    the reference's own headers (fifo.h / convert.h / demod_2400.h, not copied here);
 *                               its output is recorded in tests/golden/reference_boundary.json (make_reference_records.py)
 * so that the layout test runs on a checkout that has no reference tree beside it. */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef DUMP_REFERENCE
#include "fifo.h"
#include "convert.h"
#include "demod_2400.h"
typedef struct mag_buf buf_t;
typedef mag_buf_flags flags_t;
typedef input_format_t format_t;
#define V_DISCONTINUOUS MAGBUF_DISCONTINUOUS
#define V_UC8 INPUT_UC8
#define V_SC16 INPUT_SC16
#define V_SC16Q11 INPUT_SC16Q11
#else
#include "modes_hip_readsb.h"
typedef struct msd_mag_buf buf_t;
typedef msd_mag_buf_flags flags_t;
typedef msd_input_format_t format_t;
#define V_DISCONTINUOUS MSD_MAGBUF_DISCONTINUOUS
#define V_UC8 MSD_INPUT_UC8
#define V_SC16 MSD_INPUT_SC16
#define V_SC16Q11 MSD_INPUT_SC16Q11
#endif

#define FIELD(f) printf("\"%s\": [%zu, %zu], ", #f, offsetof(buf_t, f), sizeof(((buf_t *)0)->f))

int main(void)
{
    printf("{\"fields\": {");
    FIELD(data);
    FIELD(totalLength);
    FIELD(validLength);
    FIELD(overlap);
    FIELD(sampleTimestamp);
    FIELD(sysTimestamp);
    FIELD(flags);
    FIELD(mean_level);
    FIELD(mean_power);
    FIELD(dropped);
    printf("\"next\": [%zu, %zu]}, ", offsetof(buf_t, next), sizeof(((buf_t *)0)->next));
    printf("\"sizeof\": %zu, \"alignof\": %zu, ", sizeof(buf_t), _Alignof(buf_t));
    printf("\"MAGBUF_DISCONTINUOUS\": %d, \"sizeof_flags\": %zu, ", (int)V_DISCONTINUOUS, sizeof(flags_t));
    printf("\"INPUT_UC8\": %d, \"INPUT_SC16\": %d, \"INPUT_SC16Q11\": %d, \"sizeof_input_format\": %zu",
           (int)V_UC8, (int)V_SC16, (int)V_SC16Q11, sizeof(format_t));
#ifdef DUMP_REFERENCE
    printf(", \"PREAMBLE_THRESHOLD_DEFAULT\": %d, \"PREAMBLE_THRESHOLD_MIN\": %d, \"PREAMBLE_THRESHOLD_MAX\": %d, "
           "\"PREAMBLE_THRESHOLD_PIZERO\": %d",
           PREAMBLE_THRESHOLD_DEFAULT, PREAMBLE_THRESHOLD_MIN, PREAMBLE_THRESHOLD_MAX, PREAMBLE_THRESHOLD_PIZERO);
#endif
    printf("}\n");
    return 0;
}
