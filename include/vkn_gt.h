/* vkn_gt.h — C ABI of libvkn.so, fourth part: the ground truth of a training step.
 *
 * Conventions, error codes and the status word are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory
 * (the few HOST arrays are marked), nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation,
 * 0 = VKN_OK.  Every entry refuses before any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a shape outside the
 * envelope -> VKN_E_SHAPE, a misaligned pointer -> VKN_E_ALIGN, a host pointer where device memory is expected -> VKN_E_ARG.
 * The pointers and counts inside the per-image array (NULL masks / sem / classes, negative G / n_sem -> VKN_E_ARG) are checked once B
 * is known to lie in [1, VKN_GT_MAX_IMAGES], so that imgs[b] is indexed safely: a B outside that range is VKN_E_SHAPE whatever the
 * array holds.  The device-memory look-up comes last because it is the only check that asks the runtime.
 *
 * What it replaces: the start of `forward_train` — `preprocess_gt_masks` (knet/video/knet_quansi_dense_embed_fc_joint_train.py:152-223,
 * the same method in knet/det/knet.py) with `sem2ins_masks*` (knet/det/utils.py:8-93), and the `gt_match_indices` loop (:323-331).
 *
 * The arithmetic: `F.interpolate(..., bilinear, align_corners=False)` from [Hp, Wp] to [Hp / s, Wp / s] at an even integer s reads the
 * source at s d + s / 2 - 0.5: every output is the mean of the 2 x 2 centre pixels (s d + s / 2 - 1, s d + s / 2) of its s x s cell,
 * weights 1/4.  For byte inputs the sum is at most 1020: exact in fp32 in any order.  s = 1 is the identity.
 */
#ifndef VKN_GT_H
#define VKN_GT_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_GT_MAX_IMAGES 64    /* images per call */
#define VKN_GT_MAX_CLASSES 256  /* semantic classes: the values of a byte; also the capacity of a row of the class lists */
#define VKN_GT_MAX_IDS 1024     /* instance ids per image and side (vkn_gt_match_indices) */

/* One image of the batch (a HOST array of these, as VknTailImage is used).
 *   masks    uint8 [G][Hm][Wm]: the instance masks, NOT padded (any byte value counts as itself); may be NULL when G == 0;
 *   sem      the semantic map [Hp][Wp], uint8 or int64 (the call's `sem_i64`); NULL: the image has no semantic map;
 *   classes  vkn_gt_bank_fill_f32 only: uint8 [n_sem], the image's row of vkn_gt_classes' class lists; may be NULL when n_sem == 0;
 *   valid_h, valid_w: `img_shape`; map pixels with row >= valid_h or col >= valid_w count as the ignore label (the reference overwrites
 *            them, :171-174; here it is a predicate and the map is only read);
 *   n_sem    vkn_gt_bank_fill_f32 only: the image's number of stuff rows (what vkn_gt_classes counted);
 *   row0, sem_row0: vkn_gt_bank_fill_f32 only: the first bank row of the image's thing / stuff rows. */
typedef struct VknGtImage {
    const unsigned char* masks;
    const void* sem;
    const unsigned char* classes;
    int G, Hm, Wm;
    int valid_h, valid_w;
    int n_sem;
    int row0, sem_row0;
} VknGtImage;
size_t vkn_sizeof_gt_image(void);

/* ---- class presence and stuff labels (a clear + 2 launches).
 *      in : imgs HOST [B] (sem, valid_h, valid_w are read); sem_i64: 0 = uint8 maps, 1 = int64 maps;
 *           label_of_class HOST int [256]: the label of semantic class c, or -1: skip it (the ignore label, the thing classes).  One table
 *           expresses the three `sem2ins_masks*` variants.  It travels as a kernel argument;
 *           flags uint32 [B][8]: scratch for the presence bits (cleared by the call).
 *      The presence pass reads the valid part of every map once; a workgroup collects the classes it meets as 256 bits in LDS and
 *      publishes them with integer atomicOr: order-independent, deterministic.  The finishing launch (one workgroup per image) writes
 *      out: n_sem int32 [B], classes uint8 [B][256] (the listed classes ascending — the order of `torch.unique`; the rest of a row is not
 *           written), labels int64 [B][256] (label_of_class of the same entries);
 *           status: VKN_STATUS_RANGE is ORed into it when an int64 map holds a value outside [0, 255]; such a pixel counts as ignore.
 *      Envelope: 1 <= B <= VKN_GT_MAX_IMAGES, 1 <= Hp <= 524280, 1 <= Wp, Hp * Wp < 2^31, 0 <= valid_h <= Hp, 0 <= valid_w <= Wp; flags, n_sem
 *      4-byte, labels and int64 maps 8-byte aligned (VKN_E_ALIGN). */
int vkn_gt_classes(const VknGtImage* imgs, int B, int Hp, int Wp, int sem_i64, const int* label_of_class, unsigned* flags, int* n_sem,
                   unsigned char* classes, int64_t* labels, int* status, void* stream);

/* ---- bank fill (1 launch): the fp32 bank [G_total][Hp / s][Wp / s] in the row order of the training tail — per image its G thing
 *      rows (row0 ...), then its n_sem stuff rows in ascending class order (sem_row0 ...).
 *      thing row g: the 2 x 2-centre mean of masks[g], zero outside [Hm, Wm] (the reference's `F.pad`);
 *      stuff row j: (# of the 4 centre pixels equal to classes[j]) / 4 under the ignore predicate above; a workgroup reads the centre
 *      rows and columns of its map tile once and emits all n_sem rows from registers.
 *      A thread owns 4 neighbouring outputs: it loads 4 s bytes of a source row at once when the row pitch and the base allow (else
 *      byte by byte, bounds-checked) and stores 16 bytes when the address allows (else element by element).
 *      Envelope: s in {1, 2, 4, 8}, Hp % s == 0, Wp % s == 0, 0 <= G, 1 <= Hm <= Hp and 1 <= Wm <= Wp where G > 0,
 *      0 <= n_sem <= 256 (and sem, classes not NULL where n_sem > 0), the rows [row0, row0 + G) and [sem_row0, sem_row0 + n_sem)
 *      inside [0, G_total), 1 <= G_total, G_total (Hp / s) (Wp / s) 4 < 2^31, Hp / s <= 262140, 1 <= B <= VKN_GT_MAX_IMAGES, at most 65535 - B thing
 *      rows; bank 16-byte aligned, int64 maps 8-byte aligned. */
int vkn_gt_bank_fill_f32(const VknGtImage* imgs, int B, int Hp, int Wp, int s, int sem_i64, float* bank, int G_total, void* stream);

/* ---- gt_match_indices (1 launch, one workgroup per image): match[key_off[b] + k] = the FIRST position of key id k of image b among
 *      that image's reference ids, else -1 (`ref_ids.index(i) if i in ref_ids else -1`).
 *      in : key_ids, ref_ids int64: the images' ids concatenated; key_len, ref_len HOST int [B]: their counts per image (0 is fine);
 *      out: match int64 [sum key_len]; match_off int64 [B + 1]: the offsets of the images in `match` — the `match` / `match_off` pair
 *           of vkn_track_loss_fwd_f32 (vkn_track_train.h).
 *      Envelope: 1 <= B <= VKN_GT_MAX_IMAGES, every count in [0, VKN_GT_MAX_IDS]; pointers 8-byte aligned.  key_ids, ref_ids and
 *      match may be NULL when their total count is 0. */
int vkn_gt_match_indices(const int64_t* key_ids, const int* key_len, const int64_t* ref_ids, const int* ref_len, int B, int64_t* match,
                         int64_t* match_off, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_GT_H */
