/* vgicp_hip_map_checkpoint.h — extension of the C ABI (vgicp_hip.h): MAP CHECKPOINT.  The device map saved as one
 * self-describing blob, packed on the device, and restored slot for slot.
 *
 * A restore puts every record back into the table slot it came from, makes every tombstone a tombstone again and gives the
 * table the size it had.  Every later call, the ones that depend on slot order included (the order of a from-map scan,
 * the order in which a level is claimed, the raw log's slot identities, the next growth of the table), then gives the bits
 * the uninterrupted session would have given.
 *
 * THE BLOB, format 1.  Little-endian; every section starts on an 8-byte boundary.
 *
 *   header, 128 bytes, reserved bytes zero:
 *       0  magic[8] = "VGICPMAP"
 *       8  u32 format = 1                 (VGICP_CHECKPOINT_FORMAT)
 *      12  u32 header_bytes = 128
 *      16  u64 total_bytes
 *      24  f64 voxel_size
 *      32  u64 slots
 *      40  u64 voxels      F
 *      48  u64 tombstones  T
 *      56  u64 raw_points  P
 *      64  u32 flags                      (bit 0, VGICP_CHECKPOINT_RAW_POINTS: the map keeps raw points)
 *      68  u32 record_bytes = 128
 *      72  u64 checksum of bytes [128, total_bytes)
 *   sections, in this order:
 *       u32 full_slots[F]      padded to 8 bytes (the pad is zero)
 *       u32 tomb_slots[T]      padded to 8 bytes
 *       records[F]             128 bytes each: key[3] i32, state i32, mean[3] f64, cov[9] f64 column-major, count u64,
 *                              spare u64
 *       f64 raw[P][3]
 *   total_bytes = 128 + pad8(4 F) + pad8(4 T) + 128 F + 24 P.
 *
 *   CHECKSUM.  Word i of the payload (bytes [128, total_bytes) as u64 words) is multiplied by 2 i + 1 and the products
 *   are summed mod 2^64.  An odd factor is a unit mod 2^64, so every single flipped bit of the payload changes the sum;
 *   two swapped words a, b at places i, j move it by (a - b) 2 (j - i), so they change it unless they are equal (or
 *   their difference ends in so many zero bits that the product is a multiple of 2^64).  It is computed on the host.
 *   It covers the payload, not the header: the header's fields are held by rules 1 - 8 below, all but voxel_size, of
 *   which rule 4 is all that is asked.
 *
 *   CANONICAL ORDER.  Two checkpoints of an unchanged map are the same bytes.  full_slots and tomb_slots ascend.
 *   records[j] is the record at full_slots[j], verbatim, with its spare word zero.  The raw section holds, for
 *   j = 0 .. F - 1 in turn, voxel j's `count` points in ordinal order: an entry's slot and ordinal (vgicp_hip_map_points.h:
 *   the voxel's table slot and the point's index in the voxel's list) are implied by its position, so only xyz is stored.
 *   The compaction is by ballots and prefix sums, never an atomic append.
 *
 *   The format depends on the table's hash and probe sequence (a key must be reachable from its home slot where the blob
 *   puts it): `format` is bumped whenever either changes.
 *
 * THE CHECK.  A pure function of the bytes (no device, no context): vgicp_map_checkpoint_info runs it, and
 * vgicp_map_restore runs it before anything else happens.  Its rules, in order; `rule` is the first that fails:
 *    1. bytes >= 128 and the magic is right;
 *    2. format, header_bytes and record_bytes have their format-1 values;
 *    3. the reserved bytes are zero and no unknown flag is set;
 *    4. voxel_size is finite and > 0;
 *    5. slots is a power of two within 1024 .. 2^32;
 *    6. 2 (F + T) <= slots, the table's load bound;
 *    7. P = 0 without the raw-points flag, and P <= 2^31;
 *    8. bytes == total_bytes == the formula;
 *    9. the checksum;
 *   10. full_slots strictly ascending and < slots;
 *   11. tomb_slots likewise;
 *   12. the two lists disjoint;
 *   13. every record's state is FULL (1), its spare word 0, its count >= 1;
 *   14. with the raw-points flag, the counts sum to P.
 * NOT checked: that a key is reachable from its home slot, that means are finite, that a covariance is symmetric.  A blob
 * that passes is SAFE to load, not necessarily meaningful.  Every index a kernel takes from the blob has passed rules
 * 10 - 14 on the host; the restore kernels still guard slot < slots and position < P.
 *
 * THE RAW STORE.  In vgicp_hip_map_points.h's terms, VGICP_OPTION_MAP_RAW_POINTS is switched only while the map holds no
 * voxel.  vgicp_map_restore is the one call that may switch it while a map exists: afterwards the context keeps raw
 * points exactly when the blob's flag says so, whatever the option was, and the store holds the blob's P points.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry points live in a library of their own beside the module,
 * libvgicp_hip_map_checkpoint.so, which links against libvgicp_hip.so and must come from the same build (a context of
 * another build is refused).  VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced.  Nothing of
 * this header is allocated before the first call.  What the calls allocate stays with the context until it is destroyed
 * and only grows: page-locked memory of 1.25 times the largest blob that went through it (about 165 MB after a map of
 * one million voxels) and the blob's sections in the context's device staging area.  Single device. */
#ifndef VGICP_HIP_MAP_CHECKPOINT_H_
#define VGICP_HIP_MAP_CHECKPOINT_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_CHECKPOINT_FORMAT 1
#define VGICP_CHECKPOINT_HEADER_BYTES 128
#define VGICP_CHECKPOINT_RECORD_BYTES 128
#define VGICP_CHECKPOINT_RAW_POINTS 1u   /* flags, bit 0 */
#define VGICP_CHECKPOINT_RULES 14

typedef struct vgicp_checkpoint_info {   /* 80 bytes, LP64: the header's fields, then the check's verdict */
  uint32_t format, header_bytes;
  uint64_t total_bytes;
  double   voxel_size;
  uint64_t slots, voxels, tombstones, raw_points;
  uint32_t flags, record_bytes;
  uint64_t checksum;
  int32_t  rule, reserved;   /* 0: the blob passes; else the number of the first rule it fails; 0 */
} vgicp_checkpoint_info;

typedef struct vgicp_checkpoint_stats {   /* 56 bytes, LP64 */
  uint64_t bytes;                       /* of the blob */
  uint64_t voxels, tombstones, raw_points;
  int32_t  launches, reserved;          /* kernel launches of this call; 0 */
  double   seconds, device_seconds;     /* host wall time of the call; event span around its launches and copies */
} vgicp_checkpoint_stats;

/* *bytes = what vgicp_map_checkpoint would write now.  Settles what is pending.  With raw points on, one launch and
 * one synchronisation count them.  VGICP_ERR_BAD_ARGUMENT: NULL ctx or bytes, a context of another build, several
 * devices; VGICP_ERR_NOT_READY: no map. */
int vgicp_map_checkpoint_size(vgicp_ctx* ctx, size_t* bytes);

/* The map as a blob.  Settles what is pending; otherwise read-only: the map, its version, the resident scan, the totals
 * and the counters are untouched.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated:
 *    1. NULL ctx, blob or written;
 *    2. ctx was not made by this build of the module;
 *    3. ctx is a multi-device context (vgicp_create_multi), has a communicator or is peer-connected;
 *    4. no map (VGICP_ERR_NOT_READY);
 *    5. capacity below the size: *written = the size and nothing is copied.
 * An empty map gives a valid blob of 128 bytes.
 *
 * LAUNCHES, with ONE host synchronisation behind them.  MARK: one lane per slot reads the record's key and state; a wave
 * stores two ballots, FULL and TOMB; a workgroup its two counts and, with raw points on, the sum of its FULL records'
 * counts.  SCAN: one workgroup takes the exclusive prefix sums over the workgroups' counts and the totals.  EMIT: the two
 * slot lists, the records (eight lanes per record, whole lines) and, with raw points on, every FULL slot's offset into the
 * raw section: the exclusive prefix sum of the counts in record order.  With raw points on, SCATTER: every live entry of
 * the log to offset[slot] + ordinal.  The bytes reach `blob` through page-locked memory of the context's own: the
 * runtime never sees the caller's pages. */
int vgicp_map_checkpoint(vgicp_ctx* ctx, size_t capacity, void* blob, size_t* written,
                         vgicp_checkpoint_stats* stats /* optional */);

/* HOST ONLY: the header of a blob and the check's verdict.  VGICP_OK and info->rule == 0 when the blob passes;
 * VGICP_ERR_BAD_ARGUMENT with info->rule set (and the header's fields as far as rule 1 let them be read) when it does
 * not, or with NULL blob or info.  The text (vgicp_last_error of a NULL context) names the rule. */
int vgicp_map_checkpoint_info(const void* blob, size_t bytes, vgicp_checkpoint_info* info);

/* The map of ctx becomes the blob's.  stats is optional.
 *
 * REFUSALS, in this order, all VGICP_ERR_BAD_ARGUMENT.  A refused restore changes nothing in the context:
 *    1. NULL ctx or blob;
 *    2. ctx was not made by this build of the module;
 *    3. several devices, as above;
 *    4. the first rule of the check that fails; the text names it.
 * Otherwise what is pending is settled, the new table (and the raw log if the blob asks for one) is allocated BEFORE the
 * old ones are let go (a failed allocation leaves the old map in place), the blob goes to the device through page-locked
 * staging memory of the library's own, the table is cleared to EMPTY, SCATTER writes the records to their slots (eight
 * lanes per record) and the tombstones' states, and with raw points the log is rebuilt in canonical order: the entry at
 * offset[j] + o is {xyz, full_slots[j], o}.  ONE host synchronisation.
 *
 * Afterwards every FULL record is byte for byte where it was, every tombstone is a tombstone (its other bytes are not
 * carried: no reader looks at them) and every other slot is EMPTY.  voxel_size, the table's size, the voxel and tombstone
 * counts and the raw store come from the header.  The map's version advances, so the dense copy and every requested level
 * are rebuilt lazily.  UNTOUCHED: the resident scan and its generation, the requested number of levels, the gated and
 * carve totals, the counters, every option. */
int vgicp_map_restore(vgicp_ctx* ctx, const void* blob, size_t bytes, vgicp_checkpoint_stats* stats /* optional */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_CHECKPOINT_H_ */
