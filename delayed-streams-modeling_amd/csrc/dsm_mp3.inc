// dsm_mp3.inc — MPEG-1 Audio Layer III decoder + windowed-sinc resampler, host side (included by dsm_audio.inc; no device work).
//
// What it stands in for: srv/utils.rs:263-305 `pcm_decode` (symphonia: probe the container, decode every packet of the first
// audio track, keep CHANNEL 0 as f32) for the bodies the reference's own samples use — audio/bria.mp3 (BASELINE.json configs[0]),
// loona.mp3, sample_fr_hibiki_*.mp3: MPEG-1 Layer III, 44.1 kHz — and srv/batched_asr.rs:834-842 `kaudio::resample(&pcm, rate,
// 24000)`.  symphonia and kaudio are un-vendored crates and nothing that decodes mp3 is importable offline, so this follows the
// published algorithm (ISO/IEC 11172-3: header, side information, bit reservoir, scale factors, Huffman tables B.7, requantisation,
// MS / intensity stereo, reordering, alias reduction, IMDCT with window switching, polyphase synthesis with window B.3) and its
// output is PARITY-UNPINNED against symphonia (decoders differ in the last bits of the float pipeline).  What IS pinned
// (tests/test_mp3.py): the Huffman tables are complete prefix codes over every (x, y); analysis + this synthesis bank
// reconstructs a signal to > 80 dB; IMDCT + overlap-add inverts an MDCT; on every mp3 the reference ships the frame walk loses
// sync nowhere, every granule's Huffman data ends inside its part2_3_length, and the PCM is band-limited speech.
// Not built: MPEG-2 / 2.5 (LSF) streams, Layers I / II, free-format bit rates, CRC verification (the check word is skipped).
// Intensity stereo follows the standard's text but no sample exercises it (all five files are mono).
#include <math.h>
#include "dsm_pcm_format.h"  // guarded: the phase table of the resampler, shared with the per-slot ingest and egress

namespace dsm_mp3 {

// ---- ISO/IEC 11172-3 Table B.7 as (code, length), index x * 16^... = x * ylen + y ------------------------------------------------
struct HuffDef { int xlen, linbits; const uint16_t* code; const uint8_t* len; };
static const uint16_t hc1[] = {1, 1, 1, 0};
static const uint8_t hl1[] = {1, 3, 2, 3};
static const uint16_t hc2[] = {1, 2, 1, 3, 1, 1, 3, 2, 0};
static const uint8_t hl2[] = {1, 3, 6, 3, 3, 5, 5, 5, 6};
static const uint16_t hc3[] = {3, 2, 1, 1, 1, 1, 3, 2, 0};
static const uint8_t hl3[] = {2, 2, 6, 3, 2, 5, 5, 5, 6};
static const uint16_t hc5[] = {1, 2, 6, 5, 3, 1, 4, 4, 7, 5, 7, 1, 6, 1, 1, 0};
static const uint8_t hl5[] = {1, 3, 6, 7, 3, 3, 6, 7, 6, 6, 7, 8, 7, 6, 7, 8};
static const uint16_t hc6[] = {7, 3, 5, 1, 6, 2, 3, 2, 5, 4, 4, 1, 3, 3, 2, 0};
static const uint8_t hl6[] = {3, 3, 5, 7, 3, 2, 4, 5, 4, 4, 5, 6, 6, 5, 6, 7};
static const uint16_t hc7[] = {1, 2, 10, 19, 16, 10, 3, 3, 7, 10, 5, 3, 11, 4, 13, 17, 8, 4, 12, 11, 18, 15, 11, 2, 7, 6, 9, 14, 3, 1, 6, 4, 5, 3, 2, 0};
static const uint8_t hl7[] = {1, 3, 6, 8, 8, 9, 3, 4, 6, 7, 7, 8, 6, 5, 7, 8, 8, 9, 7, 7, 8, 9, 9, 9, 7, 7, 8, 9, 9, 10, 8, 8, 9, 10, 10, 10};
static const uint16_t hc8[] = {3, 4, 6, 18, 12, 5, 5, 1, 2, 16, 9, 3, 7, 3, 5, 14, 7, 3, 19, 17, 15, 13, 10, 4, 13, 5, 8, 11, 5, 1, 12, 4, 4, 1, 1, 0};
static const uint8_t hl8[] = {2, 3, 6, 8, 8, 9, 3, 2, 4, 8, 8, 8, 6, 4, 6, 8, 8, 9, 8, 8, 8, 9, 9, 10, 8, 7, 8, 9, 10, 10, 9, 8, 9, 9, 11, 11};
static const uint16_t hc9[] = {7, 5, 9, 14, 15, 7, 6, 4, 5, 5, 6, 7, 7, 6, 8, 8, 8, 5, 15, 6, 9, 10, 5, 1, 11, 7, 9, 6, 4, 1, 14, 4, 6, 2, 6, 0};
static const uint8_t hl9[] = {3, 3, 5, 6, 8, 9, 3, 3, 4, 5, 6, 8, 4, 4, 5, 6, 7, 8, 6, 5, 6, 7, 7, 8, 7, 6, 7, 7, 8, 9, 8, 7, 8, 8, 9, 9};
static const uint16_t hc10[] = {1, 2, 10, 23, 35, 30, 12, 17, 3, 3, 8, 12, 18, 21, 12, 7, 11, 9, 15, 21, 32, 40, 19, 6, 14, 13, 22, 34, 46, 23, 18, 7, 20, 19, 33, 47, 27, 22, 9, 3, 31, 22, 41, 26, 21, 20, 5, 3, 14, 13, 10, 11, 16, 6, 5, 1, 9, 8, 7, 8, 4, 4, 2, 0};
static const uint8_t hl10[] = {1, 3, 6, 8, 9, 9, 9, 10, 3, 4, 6, 7, 8, 9, 8, 8, 6, 6, 7, 8, 9, 10, 9, 9, 7, 7, 8, 9, 10, 10, 9, 10, 8, 8, 9, 10, 10, 10, 10, 10, 9, 9, 10, 10, 11, 11, 10, 11, 8, 8, 9, 10, 10, 10, 11, 11, 9, 8, 9, 10, 10, 11, 11, 11};
static const uint16_t hc11[] = {3, 4, 10, 24, 34, 33, 21, 15, 5, 3, 4, 10, 32, 17, 11, 10, 11, 7, 13, 18, 30, 31, 20, 5, 25, 11, 19, 59, 27, 18, 12, 5, 35, 33, 31, 58, 30, 16, 7, 5, 28, 26, 32, 19, 17, 15, 8, 14, 14, 12, 9, 13, 14, 9, 4, 1, 11, 4, 6, 6, 6, 3, 2, 0};
static const uint8_t hl11[] = {2, 3, 5, 7, 8, 9, 8, 9, 3, 3, 4, 6, 8, 8, 7, 8, 5, 5, 6, 7, 8, 9, 8, 8, 7, 6, 7, 9, 8, 10, 8, 9, 8, 8, 8, 9, 9, 10, 9, 10, 8, 8, 9, 10, 10, 11, 10, 11, 8, 7, 7, 8, 9, 10, 10, 10, 8, 7, 8, 9, 10, 10, 10, 10};
static const uint16_t hc12[] = {9, 6, 16, 33, 41, 39, 38, 26, 7, 5, 6, 9, 23, 16, 26, 11, 17, 7, 11, 14, 21, 30, 10, 7, 17, 10, 15, 12, 18, 28, 14, 5, 32, 13, 22, 19, 18, 16, 9, 5, 40, 17, 31, 29, 17, 13, 4, 2, 27, 12, 11, 15, 10, 7, 4, 1, 27, 12, 8, 12, 6, 3, 1, 0};
static const uint8_t hl12[] = {4, 3, 5, 7, 8, 9, 9, 9, 3, 3, 4, 5, 7, 7, 8, 8, 5, 4, 5, 6, 7, 8, 7, 8, 6, 5, 6, 6, 7, 8, 8, 8, 7, 6, 7, 7, 8, 8, 8, 9, 8, 7, 8, 8, 8, 9, 8, 9, 8, 7, 7, 8, 8, 9, 9, 10, 9, 8, 8, 9, 9, 9, 9, 10};
static const uint16_t hc13[] = {1, 5, 14, 21, 34, 51, 46, 71, 42, 52, 68, 52, 67, 44, 43, 19, 3, 4, 12, 19, 31, 26, 44, 33, 31, 24, 32, 24, 31, 35, 22, 14, 15, 13, 23, 36, 59, 49, 77, 65, 29, 40, 30, 40, 27, 33, 42, 16, 22, 20, 37, 61, 56, 79, 73, 64, 43, 76, 56, 37, 26, 31, 25, 14, 35, 16, 60, 57, 97, 75, 114, 91, 54, 73, 55, 41, 48, 53, 23, 24, 58, 27, 50, 96, 76, 70, 93, 84, 77, 58, 79, 29, 74, 49, 41, 17, 47, 45, 78, 74, 115, 94, 90, 79, 69, 83, 71, 50, 59, 38, 36, 15, 72, 34, 56, 95, 92, 85, 91, 90, 86, 73, 77, 65, 51, 44, 43, 42, 43, 20, 30, 44, 55, 78, 72, 87, 78, 61, 46, 54, 37, 30, 20, 16, 53, 25, 41, 37, 44, 59, 54, 81, 66, 76, 57, 54, 37, 18, 39, 11, 35, 33, 31, 57, 42, 82, 72, 80, 47, 58, 55, 21, 22, 26, 38, 22, 53, 25, 23, 38, 70, 60, 51, 36, 55, 26, 34, 23, 27, 14, 9, 7, 34, 32, 28, 39, 49, 75, 30, 52, 48, 40, 52, 28, 18, 17, 9, 5, 45, 21, 34, 64, 56, 50, 49, 45, 31, 19, 12, 15, 10, 7, 6, 3, 48, 23, 20, 39, 36, 35, 53, 21, 16, 23, 13, 10, 6, 1, 4, 2, 16, 15, 17, 27, 25, 20, 29, 11, 17, 12, 16, 8, 1, 1, 0, 1};
static const uint8_t hl13[] = {1, 4, 6, 7, 8, 9, 9, 10, 9, 10, 11, 11, 12, 12, 13, 13, 3, 4, 6, 7, 8, 8, 9, 9, 9, 9, 10, 10, 11, 12, 12, 12, 6, 6, 7, 8, 9, 9, 10, 10, 9, 10, 10, 11, 11, 12, 13, 13, 7, 7, 8, 9, 9, 10, 10, 10, 10, 11, 11, 11, 11, 12, 13, 13, 8, 7, 9, 9, 10, 10, 11, 11, 10, 11, 11, 12, 12, 13, 13, 14, 9, 8, 9, 10, 10, 10, 11, 11, 11, 11, 12, 11, 13, 13, 14, 14, 9, 9, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 13, 13, 14, 14, 10, 9, 10, 11, 11, 11, 12, 12, 12, 12, 13, 13, 13, 14, 16, 16, 9, 8, 9, 10, 10, 11, 11, 12, 12, 12, 12, 13, 13, 14, 15, 15, 10, 9, 10, 10, 11, 11, 11, 13, 12, 13, 13, 14, 14, 14, 16, 15, 10, 10, 10, 11, 11, 12, 12, 13, 12, 13, 14, 13, 14, 15, 16, 17, 11, 10, 10, 11, 12, 12, 12, 12, 13, 13, 13, 14, 15, 15, 15, 16, 11, 11, 11, 12, 12, 13, 12, 13, 14, 14, 15, 15, 15, 16, 16, 16, 12, 11, 12, 13, 13, 13, 14, 14, 14, 14, 14, 15, 16, 15, 16, 16, 13, 12, 12, 13, 13, 13, 15, 14, 14, 17, 15, 15, 15, 17, 16, 16, 12, 12, 13, 14, 14, 14, 15, 14, 15, 15, 16, 16, 19, 18, 19, 16};
static const uint16_t hc15[] = {7, 12, 18, 53, 47, 76, 124, 108, 89, 123, 108, 119, 107, 81, 122, 63, 13, 5, 16, 27, 46, 36, 61, 51, 42, 70, 52, 83, 65, 41, 59, 36, 19, 17, 15, 24, 41, 34, 59, 48, 40, 64, 50, 78, 62, 80, 56, 33, 29, 28, 25, 43, 39, 63, 55, 93, 76, 59, 93, 72, 54, 75, 50, 29, 52, 22, 42, 40, 67, 57, 95, 79, 72, 57, 89, 69, 49, 66, 46, 27, 77, 37, 35, 66, 58, 52, 91, 74, 62, 48, 79, 63, 90, 62, 40, 38, 125, 32, 60, 56, 50, 92, 78, 65, 55, 87, 71, 51, 73, 51, 70, 30, 109, 53, 49, 94, 88, 75, 66, 122, 91, 73, 56, 42, 64, 44, 21, 25, 90, 43, 41, 77, 73, 63, 56, 92, 77, 66, 47, 67, 48, 53, 36, 20, 71, 34, 67, 60, 58, 49, 88, 76, 67, 106, 71, 54, 38, 39, 23, 15, 109, 53, 51, 47, 90, 82, 58, 57, 48, 72, 57, 41, 23, 27, 62, 9, 86, 42, 40, 37, 70, 64, 52, 43, 70, 55, 42, 25, 29, 18, 11, 11, 118, 68, 30, 55, 50, 46, 74, 65, 49, 39, 24, 16, 22, 13, 14, 7, 91, 44, 39, 38, 34, 63, 52, 45, 31, 52, 28, 19, 14, 8, 9, 3, 123, 60, 58, 53, 47, 43, 32, 22, 37, 24, 17, 12, 15, 10, 2, 1, 71, 37, 34, 30, 28, 20, 17, 26, 21, 16, 10, 6, 8, 6, 2, 0};
static const uint8_t hl15[] = {3, 4, 5, 7, 7, 8, 9, 9, 9, 10, 10, 11, 11, 11, 12, 13, 4, 3, 5, 6, 7, 7, 8, 8, 8, 9, 9, 10, 10, 10, 11, 11, 5, 5, 5, 6, 7, 7, 8, 8, 8, 9, 9, 10, 10, 11, 11, 11, 6, 6, 6, 7, 7, 8, 8, 9, 9, 9, 10, 10, 10, 11, 11, 11, 7, 6, 7, 7, 8, 8, 9, 9, 9, 9, 10, 10, 10, 11, 11, 11, 8, 7, 7, 8, 8, 8, 9, 9, 9, 9, 10, 10, 11, 11, 11, 12, 9, 7, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 11, 11, 12, 12, 9, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 11, 11, 11, 12, 9, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 12, 12, 12, 9, 8, 9, 9, 9, 9, 10, 10, 10, 11, 11, 11, 11, 12, 12, 12, 10, 9, 9, 9, 10, 10, 10, 10, 10, 11, 11, 11, 11, 12, 13, 12, 10, 9, 9, 9, 10, 10, 10, 10, 11, 11, 11, 11, 12, 12, 12, 13, 11, 10, 9, 10, 10, 10, 11, 11, 11, 11, 11, 11, 12, 12, 13, 13, 11, 10, 10, 10, 10, 11, 11, 11, 11, 12, 12, 12, 12, 12, 13, 13, 12, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 13, 13, 12, 13, 12, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 13, 13, 13, 13};
static const uint16_t hc16[] = {1, 5, 14, 44, 74, 63, 110, 93, 172, 149, 138, 242, 225, 195, 376, 17, 3, 4, 12, 20, 35, 62, 53, 47, 83, 75, 68, 119, 201, 107, 207, 9, 15, 13, 23, 38, 67, 58, 103, 90, 161, 72, 127, 117, 110, 209, 206, 16, 45, 21, 39, 69, 64, 114, 99, 87, 158, 140, 252, 212, 199, 387, 365, 26, 75, 36, 68, 65, 115, 101, 179, 164, 155, 264, 246, 226, 395, 382, 362, 9, 66, 30, 59, 56, 102, 185, 173, 265, 142, 253, 232, 400, 388, 378, 445, 16, 111, 54, 52, 100, 184, 178, 160, 133, 257, 244, 228, 217, 385, 366, 715, 10, 98, 48, 91, 88, 165, 157, 148, 261, 248, 407, 397, 372, 380, 889, 884, 8, 85, 84, 81, 159, 156, 143, 260, 249, 427, 401, 392, 383, 727, 713, 708, 7, 154, 76, 73, 141, 131, 256, 245, 426, 406, 394, 384, 735, 359, 710, 352, 11, 139, 129, 67, 125, 247, 233, 229, 219, 393, 743, 737, 720, 885, 882, 439, 4, 243, 120, 118, 115, 227, 223, 396, 746, 742, 736, 721, 712, 706, 223, 436, 6, 202, 224, 222, 218, 216, 389, 386, 381, 364, 888, 443, 707, 440, 437, 1728, 4, 747, 211, 210, 208, 370, 379, 734, 723, 714, 1735, 883, 877, 876, 3459, 865, 2, 377, 369, 102, 187, 726, 722, 358, 711, 709, 866, 1734, 871, 3458, 870, 434, 0, 12, 10, 7, 11, 10, 17, 11, 9, 13, 12, 10, 7, 5, 3, 1, 3};
static const uint8_t hl16[] = {1, 4, 6, 8, 9, 9, 10, 10, 11, 11, 11, 12, 12, 12, 13, 9, 3, 4, 6, 7, 8, 9, 9, 9, 10, 10, 10, 11, 12, 11, 12, 8, 6, 6, 7, 8, 9, 9, 10, 10, 11, 10, 11, 11, 11, 12, 12, 9, 8, 7, 8, 9, 9, 10, 10, 10, 11, 11, 12, 12, 12, 13, 13, 10, 9, 8, 9, 9, 10, 10, 11, 11, 11, 12, 12, 12, 13, 13, 13, 9, 9, 8, 9, 9, 10, 11, 11, 12, 11, 12, 12, 13, 13, 13, 14, 10, 10, 9, 9, 10, 11, 11, 11, 11, 12, 12, 12, 12, 13, 13, 14, 10, 10, 9, 10, 10, 11, 11, 11, 12, 12, 13, 13, 13, 13, 15, 15, 10, 10, 10, 10, 11, 11, 11, 12, 12, 13, 13, 13, 13, 14, 14, 14, 10, 11, 10, 10, 11, 11, 12, 12, 13, 13, 13, 13, 14, 13, 14, 13, 11, 11, 11, 10, 11, 12, 12, 12, 12, 13, 14, 14, 14, 15, 15, 14, 10, 12, 11, 11, 11, 12, 12, 13, 14, 14, 14, 14, 14, 14, 13, 14, 11, 12, 12, 12, 12, 12, 13, 13, 13, 13, 15, 14, 14, 14, 14, 16, 11, 14, 12, 12, 12, 13, 13, 14, 14, 14, 16, 15, 15, 15, 17, 15, 11, 13, 13, 11, 12, 14, 14, 13, 14, 14, 15, 16, 15, 17, 15, 14, 11, 9, 8, 8, 9, 9, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 8};
static const uint16_t hc24[] = {15, 13, 46, 80, 146, 262, 248, 434, 426, 669, 653, 649, 621, 517, 1032, 88, 14, 12, 21, 38, 71, 130, 122, 216, 209, 198, 327, 345, 319, 297, 279, 42, 47, 22, 41, 74, 68, 128, 120, 221, 207, 194, 182, 340, 315, 295, 541, 18, 81, 39, 75, 70, 134, 125, 116, 220, 204, 190, 178, 325, 311, 293, 271, 16, 147, 72, 69, 135, 127, 118, 112, 210, 200, 188, 352, 323, 306, 285, 540, 14, 263, 66, 129, 126, 119, 114, 214, 202, 192, 180, 341, 317, 301, 281, 262, 12, 249, 123, 121, 117, 113, 215, 206, 195, 185, 347, 330, 308, 291, 272, 520, 10, 435, 115, 111, 109, 211, 203, 196, 187, 353, 332, 313, 298, 283, 531, 381, 17, 427, 212, 208, 205, 201, 193, 186, 177, 169, 320, 303, 286, 268, 514, 377, 16, 335, 199, 197, 191, 189, 181, 174, 333, 321, 305, 289, 275, 521, 379, 371, 11, 668, 184, 183, 179, 175, 344, 331, 314, 304, 290, 277, 530, 383, 373, 366, 10, 652, 346, 171, 168, 164, 318, 309, 299, 287, 276, 263, 513, 375, 368, 362, 6, 648, 322, 316, 312, 307, 302, 292, 284, 269, 261, 512, 376, 370, 364, 359, 4, 620, 300, 296, 294, 288, 282, 273, 266, 515, 380, 374, 369, 365, 361, 357, 2, 1033, 280, 278, 274, 267, 264, 259, 382, 378, 372, 367, 363, 360, 358, 356, 0, 43, 20, 19, 17, 15, 13, 11, 9, 7, 6, 4, 7, 5, 3, 1, 3};
static const uint8_t hl24[] = {4, 4, 6, 7, 8, 9, 9, 10, 10, 11, 11, 11, 11, 11, 12, 9, 4, 4, 5, 6, 7, 8, 8, 9, 9, 9, 10, 10, 10, 10, 10, 8, 6, 5, 6, 7, 7, 8, 8, 9, 9, 9, 9, 10, 10, 10, 11, 7, 7, 6, 7, 7, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 7, 8, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10, 10, 10, 11, 7, 9, 7, 8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 7, 9, 8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 11, 7, 10, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 11, 11, 8, 10, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 8, 10, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 11, 11, 11, 8, 11, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 8, 11, 10, 9, 9, 9, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 8, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 8, 11, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 8, 12, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 8, 8, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 4};
static const uint16_t hcA[] = {1, 5, 4, 5, 6, 5, 4, 4, 7, 3, 6, 0, 7, 2, 3, 1};   // count1 table A, index v w x y
static const uint8_t hlA[] = {1, 4, 4, 5, 4, 6, 5, 6, 4, 5, 5, 6, 5, 6, 6, 6};
static const uint16_t hcB[] = {15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0};
static const uint8_t hlB[] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
// table_select 0..31 (4 and 14 are not used by the standard; 16..23 share table 16's codes, 24..31 table 24's)
static const HuffDef kHuff[34] = {
    {0, 0, nullptr, nullptr}, {2, 0, hc1, hl1}, {3, 0, hc2, hl2}, {3, 0, hc3, hl3}, {0, 0, nullptr, nullptr}, {4, 0, hc5, hl5},
    {4, 0, hc6, hl6}, {6, 0, hc7, hl7}, {6, 0, hc8, hl8}, {6, 0, hc9, hl9}, {8, 0, hc10, hl10}, {8, 0, hc11, hl11},
    {8, 0, hc12, hl12}, {16, 0, hc13, hl13}, {0, 0, nullptr, nullptr}, {16, 0, hc15, hl15},
    {16, 1, hc16, hl16}, {16, 2, hc16, hl16}, {16, 3, hc16, hl16}, {16, 4, hc16, hl16}, {16, 6, hc16, hl16}, {16, 8, hc16, hl16},
    {16, 10, hc16, hl16}, {16, 13, hc16, hl16}, {16, 4, hc24, hl24}, {16, 5, hc24, hl24}, {16, 6, hc24, hl24}, {16, 7, hc24, hl24},
    {16, 8, hc24, hl24}, {16, 9, hc24, hl24}, {16, 11, hc24, hl24}, {16, 13, hc24, hl24},
    {4, 0, hcA, hlA}, {4, 0, hcB, hlB}};  // 32, 33: the count1 tables as 4 x 4 "pairs" (v w, x y)

// scale factor band boundaries, MPEG-1 (Table B.8): [44.1, 48, 32 kHz]
static const int kSfbLong[3][23] = {
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576},
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576},
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576}};
static const int kSfbShort[3][14] = {
    {0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192},
    {0, 4, 8, 12, 16, 22, 28, 38, 50, 64, 80, 100, 126, 192},
    {0, 4, 8, 12, 16, 22, 30, 42, 58, 78, 104, 138, 180, 192}};
static const int kSlen[2][16] = {{0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4}, {0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3}};
static const int kPretab[22] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2, 0};
static const int kBitrate[15] = {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320};
static const int kRate[3] = {44100, 48000, 32000};
// Table B.3 (synthesis window D[i] x 65536): the first 257 taps of the prototype, D[i] = (-1)^(i / 64) base[i] for i <= 256 and
// (-1)^(i / 64) base[512 - i] above (the prototype is symmetric about tap 256)
static const int32_t kWinBase[257] = {
    0, -1, -1, -1, -1, -1, -1, -2, -2, -2, -2, -3, -3, -4, -4, -5, -5, -6, -7, -7, -8, -9, -10, -11, -13, -14, -16, -17, -19, -21, -24, -26,
    -29, -31, -35, -38, -41, -45, -49, -53, -58, -63, -68, -73, -79, -85, -91, -97, -104, -111, -117, -125, -132, -139, -147, -154, -161,
    -169, -176, -183, -190, -196, -202, -208, -213, -218, -222, -225, -227, -228, -228, -227, -224, -221, -215, -208, -200, -189, -177,
    -163, -146, -127, -106, -83, -57, -29, 2, 36, 72, 111, 153, 197, 244, 294, 347, 401, 459, 519, 581, 645, 711, 779, 848, 919, 991, 1064,
    1137, 1210, 1283, 1356, 1428, 1498, 1567, 1634, 1698, 1759, 1817, 1870, 1919, 1962, 2001, 2032, 2057, 2075, 2085, 2087, 2080, 2063,
    2037, 2000, 1952, 1893, 1822, 1739, 1644, 1535, 1414, 1280, 1131, 970, 794, 605, 402, 185, -45, -288, -545, -814, -1095, -1388, -1692,
    -2006, -2330, -2663, -3004, -3351, -3705, -4063, -4425, -4788, -5153, -5517, -5879, -6237, -6589, -6935, -7271, -7597, -7910, -8209,
    -8491, -8755, -8998, -9219, -9416, -9585, -9727, -9838, -9916, -9959, -9966, -9935, -9863, -9750, -9592, -9389, -9139, -8840, -8492,
    -8092, -7640, -7134, -6574, -5959, -5288, -4561, -3776, -2935, -2037, -1082, -70, 998, 2122, 3300, 4533, 5818, 7154, 8540, 9975, 11455,
    12980, 14548, 16155, 17799, 19478, 21189, 22929, 24694, 26482, 28289, 30112, 31947, 33791, 35640, 37489, 39336, 41176, 43006, 44821,
    46617, 48390, 50137, 51853, 53534, 55178, 56778, 58333, 59838, 61289, 62684, 64019, 65290, 66494, 67629, 68692, 69679, 70590, 71420,
    72169, 72835, 73415, 73908, 74313, 74630, 74856, 74992, 75038};

// ---- tables built once ----------------------------------------------------------------------------------------------------
struct Tables {
  std::vector<int16_t> tree[34];  // binary decoding trees: node n -> children tree[2 n], tree[2 n + 1]; <= 0: leaf -(x << 4 | y) - ... (see build)
  float pow43[8207];
  float syn_win[512];
  float syn_cos[64][32];
  float imdct_win[4][36];
  float imdct_cos36[36][18], imdct_cos12[12][6];
  float cs[8], ca[8];
  float is_ratio[7][2];
  Tables() {
    for (int t = 0; t < 34; ++t) {
      const HuffDef& h = kHuff[t];
      if (!h.code) continue;
      std::vector<int16_t>& tr = tree[t];
      tr.assign(2, 0);  // root = node 0; entry 0 = "no child yet"; a leaf for value v is stored as -(v + 1); an inner node n as +n
      const int n = h.xlen * h.xlen;
      for (int i = 0; i < n; ++i) {
        int node = 0;
        for (int b = h.len[i] - 1; b >= 0; --b) {
          const int bit = (h.code[i] >> b) & 1;
          int16_t& slot = tr[2 * node + bit];
          if (b == 0) {
            slot = (int16_t)(-(((i / h.xlen) << 4 | (i % h.xlen)) + 1));
          } else {
            if (slot == 0) {
              const int nn = (int)tr.size() / 2;
              tr[2 * node + bit] = (int16_t)nn;  // (`slot` may dangle after the resize below)
              tr.resize(tr.size() + 2, 0);
              node = nn;
            } else {
              node = slot;
            }
          }
        }
      }
    }
    for (int i = 0; i < 8207; ++i) pow43[i] = (float)pow((double)i, 4.0 / 3.0);
    for (int i = 0; i < 512; ++i) {
      const int b = i <= 256 ? kWinBase[i] : kWinBase[512 - i];
      syn_win[i] = (float)(((i >> 6) & 1) ? -b : b) / 65536.0f;
    }
    for (int i = 0; i < 64; ++i)
      for (int k = 0; k < 32; ++k) syn_cos[i][k] = (float)cos((16 + i) * (2 * k + 1) * (M_PI / 64.0));
    for (int i = 0; i < 36; ++i) {
      imdct_win[0][i] = (float)sin(M_PI / 36 * (i + 0.5));
      imdct_win[1][i] = i < 18 ? (float)sin(M_PI / 36 * (i + 0.5)) : i < 24 ? 1.0f : i < 30 ? (float)sin(M_PI / 12 * (i - 18 + 0.5)) : 0.0f;
      imdct_win[3][i] = i < 6 ? 0.0f : i < 12 ? (float)sin(M_PI / 12 * (i - 6 + 0.5)) : i < 18 ? 1.0f : (float)sin(M_PI / 36 * (i + 0.5));
      imdct_win[2][i] = i < 12 ? (float)sin(M_PI / 12 * (i + 0.5)) : 0.0f;
      for (int k = 0; k < 18; ++k) imdct_cos36[i][k] = (float)cos(M_PI / 72 * (2 * i + 1 + 18) * (2 * k + 1));
    }
    for (int i = 0; i < 12; ++i)
      for (int k = 0; k < 6; ++k) imdct_cos12[i][k] = (float)cos(M_PI / 24 * (2 * i + 1 + 6) * (2 * k + 1));
    const double ci[8] = {-0.6, -0.535, -0.33, -0.185, -0.095, -0.041, -0.0142, -0.0037};
    for (int i = 0; i < 8; ++i) { cs[i] = (float)(1.0 / sqrt(1.0 + ci[i] * ci[i])); ca[i] = (float)(ci[i] / sqrt(1.0 + ci[i] * ci[i])); }
    for (int p = 0; p < 7; ++p) {  // intensity stereo: is_ratio = tan(is_pos pi / 12); left = r / (1 + r), right = 1 / (1 + r)
      if (p == 6) { is_ratio[p][0] = 1.0f; is_ratio[p][1] = 0.0f; continue; }
      const double r = tan(p * M_PI / 12.0);
      is_ratio[p][0] = (float)(r / (1.0 + r)); is_ratio[p][1] = (float)(1.0 / (1.0 + r));
    }
  }
};
static const Tables& tables() { static const Tables t; return t; }

// ---- bit reader over the main-data reservoir ----------------------------------------------------------------------------------
struct Bits {
  const uint8_t* p; size_t nbits, pos;
  uint32_t get(int n) {  // n <= 24; reads past the end return zeros (the caller checks `pos` against its budget)
    uint32_t v = 0;
    for (int i = 0; i < n; ++i, ++pos) v = (v << 1) | (pos < nbits ? ((p[pos >> 3] >> (7 - (pos & 7))) & 1u) : 0u);
    return v;
  }
};

struct Header { int rate_idx, bitrate, padding, mode, mode_ext, crc, nch, frame_bytes, side_bytes; };
// 11 sync bits, MPEG-1 (ID 11), Layer III (01), bit rate 1..14, sampling frequency 0..2
static bool parse_header(const uint8_t* h, Header* o) {
  if (h[0] != 0xFF || (h[1] & 0xFE) != 0xFA) return false;  // 1111 1111 | 111 11 01 x : sync, MPEG-1, Layer III
  const int br = h[2] >> 4, sr = (h[2] >> 2) & 3;
  if (br == 0 || br == 15 || sr == 3) return false;
  o->crc = !(h[1] & 1); o->bitrate = kBitrate[br]; o->rate_idx = sr; o->padding = (h[2] >> 1) & 1;
  o->mode = h[3] >> 6; o->mode_ext = (h[3] >> 4) & 3; o->nch = o->mode == 3 ? 1 : 2;
  o->frame_bytes = 144000 * o->bitrate / kRate[sr] + o->padding;
  o->side_bytes = o->nch == 1 ? 17 : 32;
  return true;
}

struct Granule {
  int part2_3_length, big_values, global_gain, scalefac_compress, window_switching, block_type, mixed_block;
  int table_select[3], subblock_gain[3], region0_count, region1_count, preflag, scalefac_scale, count1table_select;
  int scalefac_l[22], scalefac_s[13][3];
  int count1_end;    // index after the last decoded value of the count1 region
  int overrun_bits;  // Huffman data read beyond part2_3_length (0 on a well-formed stream)
};

struct Decoder {
  std::vector<uint8_t> reservoir;
  float overlap[2][32][18];
  float vbuf[2][1024];
  int voff[2];
  int scfsi[2][4];
  Granule gr[2][2];
  // statistics
  int frames = 0, lost_reservoir = 0, overruns = 0;
  Decoder() { memset(overlap, 0, sizeof overlap); memset(vbuf, 0, sizeof vbuf); voff[0] = voff[1] = 0; memset(scfsi, 0, sizeof scfsi); }

  static int huff_pair(const Tables& T, int t, Bits& b, int* x, int* y) {
    const std::vector<int16_t>& tr = T.tree[t];
    int node = 0;
    for (int guard = 0; guard < 24; ++guard) {
      const int16_t s = tr[2 * node + (int)b.get(1)];
      if (s < 0) { const int v = -s - 1; *x = v >> 4; *y = v & 15; return 0; }
      if (s == 0) return -1;  // not a code word (cannot happen with complete tables)
      node = s;
    }
    return -1;
  }

  void read_scalefactors(Bits& b, int ch, int g) {
    Granule& G = gr[g][ch];
    const int s1 = kSlen[0][G.scalefac_compress], s2 = kSlen[1][G.scalefac_compress];
    if (G.window_switching && G.block_type == 2) {
      memset(G.scalefac_l, 0, sizeof G.scalefac_l);
      memset(G.scalefac_s, 0, sizeof G.scalefac_s);
      int sfb0 = 0;
      if (G.mixed_block) {
        for (int sfb = 0; sfb < 8; ++sfb) G.scalefac_l[sfb] = (int)b.get(s1);
        sfb0 = 3;
      }
      for (int sfb = sfb0; sfb < 12; ++sfb)
        for (int w = 0; w < 3; ++w) G.scalefac_s[sfb][w] = (int)b.get(sfb < 6 ? s1 : s2);
    } else {
      static const int band[5] = {0, 6, 11, 16, 21};
      for (int k = 0; k < 4; ++k) {
        const bool reuse = g == 1 && scfsi[ch][k];
        for (int sfb = band[k]; sfb < band[k + 1]; ++sfb)
          G.scalefac_l[sfb] = reuse ? gr[0][ch].scalefac_l[sfb] : (int)b.get(k < 2 ? s1 : s2);
      }
      G.scalefac_l[21] = 0;
    }
  }

  void read_huffman(const Tables& T, Bits& b, size_t end, int ch, int g, int sr, int* is) {
    Granule& G = gr[g][ch];
    int r1, r2;
    if (G.window_switching && G.block_type == 2) { r1 = 36; r2 = 576; }
    else {
      r1 = kSfbLong[sr][std::min(G.region0_count + 1, 22)];
      r2 = kSfbLong[sr][std::min(G.region0_count + G.region1_count + 2, 22)];
    }
    const int bv = std::min(G.big_values * 2, 576);
    int i = 0;
    for (; i < bv; i += 2) {
      const int t = G.table_select[i < r1 ? 0 : i < r2 ? 1 : 2];
      int x = 0, y = 0;
      if (kHuff[t].code) {
        if (huff_pair(T, t, b, &x, &y)) { x = y = 0; }
        const int lb = kHuff[t].linbits;
        if (lb && x == 15) x += (int)b.get(lb);
        if (x && b.get(1)) x = -x;
        if (lb && y == 15) y += (int)b.get(lb);
        if (y && b.get(1)) y = -y;
      }
      is[i] = x; is[i + 1] = y;
    }
    G.overrun_bits = b.pos > end ? (int)(b.pos - end) : 0;  // the big_values region must fit its budget on a well-formed stream
    const int tq = 32 + G.count1table_select;
    while (i <= 572 && b.pos < end) {
      int vw = 0, xy = 0;
      if (huff_pair(T, tq, b, &vw, &xy)) break;
      int q[4] = {vw >> 1, vw & 1, xy >> 1, xy & 1};
      for (int k = 0; k < 4; ++k) if (q[k] && b.get(1)) q[k] = -1;
      if (b.pos > end) break;  // the quad ran over the granule's budget: stuffing, not data (discarded)
      for (int k = 0; k < 4; ++k) is[i + k] = q[k];
      i += 4;
    }
    G.count1_end = i;
    for (; i < 576; ++i) is[i] = 0;
    b.pos = end;
  }

  void requantize(const Tables& T, int ch, int g, int sr, const int* is, float* xr) const {
    const Granule& G = gr[g][ch];
    const double mult = G.scalefac_scale ? 1.0 : 0.5;
    auto val = [&](int v, double e) { const int a = v < 0 ? -v : v; const float m = a < 8207 ? T.pow43[a] : (float)pow((double)a, 4.0 / 3.0); const float r = (float)(m * pow(2.0, e)); return v < 0 ? -r : r; };
    const double gg = (G.global_gain - 210) / 4.0;
    int i = 0;
    const bool shortb = G.window_switching && G.block_type == 2;
    if (!shortb || G.mixed_block) {
      const int lim = shortb ? 8 : 22;  // mixed: long bands 0..7 (= the first 36 lines)
      for (int sfb = 0; sfb < lim; ++sfb) {
        const double e = gg - mult * (G.scalefac_l[sfb] + (G.preflag ? kPretab[sfb] : 0));
        for (; i < kSfbLong[sr][sfb + 1]; ++i) xr[i] = val(is[i], e);
      }
    }
    if (shortb) {
      for (int sfb = G.mixed_block ? 3 : 0; sfb < 13; ++sfb) {
        const int w0 = kSfbShort[sr][sfb], wn = kSfbShort[sr][sfb + 1] - w0;
        for (int w = 0; w < 3; ++w) {
          const double e = gg - 2.0 * G.subblock_gain[w] - mult * (sfb < 12 ? G.scalefac_s[sfb][w] : 0);
          for (int k = 0; k < wn; ++k, ++i) xr[i] = val(is[i], e);
        }
      }
    }
    for (; i < 576; ++i) xr[i] = 0.0f;
  }

  // MS and intensity stereo on one granule (both channels requantised, still in bitstream order)
  void stereo(const Tables& T, const Header& h, int g, int sr, float xr[2][576]) const {
    if (h.mode != 1) return;
    const bool ms = h.mode_ext & 2, is_on = h.mode_ext & 1;
    const Granule& R = gr[g][1];
    int is_start = 576;  // first line coded with intensity stereo: above the right channel's last non-zero line
    if (is_on) {
      int last = 575;
      while (last >= 0 && xr[1][last] == 0.0f) --last;
      is_start = last + 1;
    }
    const bool shortb = R.window_switching && R.block_type == 2;
    if (is_on && is_start < 576) {
      if (!shortb) {
        for (int sfb = 0; sfb < 22; ++sfb) {
          const int b0 = kSfbLong[sr][sfb], b1 = kSfbLong[sr][sfb + 1];
          if (b0 < is_start) continue;  // only whole bands above the boundary
          const int pos = sfb < 21 ? R.scalefac_l[sfb] : R.scalefac_l[20];
          if (pos >= 7) continue;       // illegal position: the band stays as coded (MS applies below if on)
          for (int i = b0; i < b1; ++i) { const float m = xr[0][i]; xr[0][i] = m * T.is_ratio[pos][0]; xr[1][i] = m * T.is_ratio[pos][1]; }
          is_start = std::min(is_start, b0);
        }
      } else {
        for (int sfb = R.mixed_block ? 3 : 0; sfb < 13; ++sfb) {
          const int w0 = kSfbShort[sr][sfb], wn = kSfbShort[sr][sfb + 1] - w0;
          for (int w = 0; w < 3; ++w) {
            const int b0 = 3 * w0 + w * wn;
            if (b0 < is_start) continue;
            const int pos = sfb < 12 ? R.scalefac_s[sfb][w] : R.scalefac_s[11][w];
            if (pos >= 7) continue;
            for (int i = b0; i < b0 + wn; ++i) { const float m = xr[0][i]; xr[0][i] = m * T.is_ratio[pos][0]; xr[1][i] = m * T.is_ratio[pos][1]; }
          }
        }
      }
    }
    if (ms) {
      const float k = 0.70710678118654752440f;
      const int lim = is_on ? std::min(is_start, 576) : 576;
      for (int i = 0; i < lim; ++i) { const float m = xr[0][i], s = xr[1][i]; xr[0][i] = (m + s) * k; xr[1][i] = (m - s) * k; }
    }
  }

  void hybrid(const Tables& T, int ch, int g, int sr, float* xr, float out[18][32]) {
    const Granule& G = gr[g][ch];
    const bool shortb = G.window_switching && G.block_type == 2;
    if (shortb) {  // reorder the short-window bands from (sfb, window, line) to (sfb, line, window): 3 interleaved spectra
      float tmp[576];
      memcpy(tmp, xr, sizeof tmp);
      int i = G.mixed_block ? 36 : 0;
      for (int sfb = G.mixed_block ? 3 : 0; sfb < 13; ++sfb) {
        const int w0 = kSfbShort[sr][sfb], wn = kSfbShort[sr][sfb + 1] - w0;
        for (int k = 0; k < wn; ++k)
          for (int w = 0; w < 3; ++w) xr[3 * w0 + 3 * k + w] = tmp[i + w * wn + k];
        i += 3 * wn;
      }
    }
    const int aa_bands = shortb ? (G.mixed_block ? 1 : 0) : 31;  // alias reduction between long-block subbands only
    for (int sb = 0; sb < aa_bands; ++sb)
      for (int k = 0; k < 8; ++k) {
        const int lo = 18 * sb + 17 - k, hi = 18 * (sb + 1) + k;
        const float a = xr[lo], b = xr[hi];
        xr[lo] = a * T.cs[k] - b * T.ca[k];
        xr[hi] = b * T.cs[k] + a * T.ca[k];
      }
    for (int sb = 0; sb < 32; ++sb) {
      const int bt = (G.window_switching && !(G.mixed_block && sb < 2)) ? G.block_type : 0;
      const float* X = xr + 18 * sb;
      float raw[36];
      if (bt == 2) {
        for (int i = 0; i < 36; ++i) raw[i] = 0.0f;
        for (int w = 0; w < 3; ++w)
          for (int i = 0; i < 12; ++i) {
            float s = 0.0f;
            for (int k = 0; k < 6; ++k) s += X[3 * k + w] * T.imdct_cos12[i][k];
            raw[6 * w + 6 + i] += s * T.imdct_win[2][i];
          }
      } else {
        for (int i = 0; i < 36; ++i) {
          float s = 0.0f;
          for (int k = 0; k < 18; ++k) s += X[k] * T.imdct_cos36[i][k];
          raw[i] = s * T.imdct_win[bt][i];
        }
      }
      for (int i = 0; i < 18; ++i) {
        float v = raw[i] + overlap[ch][sb][i];
        overlap[ch][sb][i] = raw[18 + i];
        if ((sb & 1) && (i & 1)) v = -v;  // frequency inversion of the odd subbands
        out[i][sb] = v;
      }
    }
  }

  void synth(const Tables& T, int ch, const float sub[18][32], float* pcm /* 576 */) {
    float* V = vbuf[ch];
    for (int s = 0; s < 18; ++s) {
      voff[ch] = (voff[ch] - 64) & 1023;
      const int o = voff[ch];
      for (int i = 0; i < 64; ++i) {
        float a = 0.0f;
        for (int k = 0; k < 32; ++k) a += T.syn_cos[i][k] * sub[s][k];
        V[(o + i) & 1023] = a;
      }
      for (int j = 0; j < 32; ++j) {
        float a = 0.0f;
        for (int i = 0; i < 8; ++i) {  // U[64 i + j] = V[128 i + j], U[64 i + 32 + j] = V[128 i + 96 + j]; out = sum U D
          a += V[(o + 128 * i + j) & 1023] * T.syn_win[64 * i + j];
          a += V[(o + 128 * i + 96 + j) & 1023] * T.syn_win[64 * i + 32 + j];
        }
        pcm[32 * s + j] = a;
      }
    }
  }

  // one frame: `frame` points at the header; appends 1152 samples of channel 0 (and of channel 1 when `right`) to the outputs
  int decode_frame(const uint8_t* frame, const Header& h, std::vector<float>* left, std::vector<float>* right) {
    const Tables& T = tables();
    const uint8_t* side = frame + 4 + (h.crc ? 2 : 0);
    Bits sb{side, (size_t)h.side_bytes * 8, 0};
    const int main_data_begin = (int)sb.get(9);
    sb.get(h.nch == 1 ? 5 : 3);
    for (int ch = 0; ch < h.nch; ++ch)
      for (int k = 0; k < 4; ++k) scfsi[ch][k] = (int)sb.get(1);
    for (int g = 0; g < 2; ++g)
      for (int ch = 0; ch < h.nch; ++ch) {
        Granule& G = gr[g][ch];
        G.part2_3_length = (int)sb.get(12); G.big_values = (int)sb.get(9); G.global_gain = (int)sb.get(8);
        G.scalefac_compress = (int)sb.get(4); G.window_switching = (int)sb.get(1);
        G.block_type = 0; G.mixed_block = 0; G.subblock_gain[0] = G.subblock_gain[1] = G.subblock_gain[2] = 0; G.table_select[2] = 0;
        if (G.window_switching) {
          G.block_type = (int)sb.get(2); G.mixed_block = (int)sb.get(1);
          G.table_select[0] = (int)sb.get(5); G.table_select[1] = (int)sb.get(5);
          for (int w = 0; w < 3; ++w) G.subblock_gain[w] = (int)sb.get(3);
          G.region0_count = (G.block_type == 2 && !G.mixed_block) ? 8 : 7;
          G.region1_count = 36;  // region 2 is empty
          if (G.block_type == 0) return -1;  // forbidden
        } else {
          for (int r = 0; r < 3; ++r) G.table_select[r] = (int)sb.get(5);
          G.region0_count = (int)sb.get(4); G.region1_count = (int)sb.get(3);
        }
        G.preflag = (int)sb.get(1); G.scalefac_scale = (int)sb.get(1); G.count1table_select = (int)sb.get(1);
      }
    // bit reservoir: this frame's main data starts main_data_begin bytes before the end of what earlier frames left
    const int hdr = 4 + (h.crc ? 2 : 0) + h.side_bytes;
    const bool have = (size_t)main_data_begin <= reservoir.size();
    std::vector<uint8_t> md;
    if (have) md.assign(reservoir.end() - main_data_begin, reservoir.end());
    md.insert(md.end(), frame + hdr, frame + h.frame_bytes);
    reservoir.insert(reservoir.end(), frame + hdr, frame + h.frame_bytes);
    if (reservoir.size() > 4096) reservoir.erase(reservoir.begin(), reservoir.end() - 2048);  // main_data_begin < 512
    frames += 1;
    const size_t base = left->size();
    left->resize(base + 1152, 0.0f);
    if (right) right->resize(base + 1152, 0.0f);
    if (!have) { lost_reservoir += 1; return 0; }  // the first frames after a seek / a cut: silence, as decoders emit
    Bits b{md.data(), md.size() * 8, 0};
    for (int g = 0; g < 2; ++g) {
      float xr[2][576];
      for (int ch = 0; ch < h.nch; ++ch) {
        Granule& G = gr[g][ch];
        const size_t start = b.pos, end = start + (size_t)G.part2_3_length;
        int is[576];
        read_scalefactors(b, ch, g);
        read_huffman(T, b, end, ch, g, h.rate_idx, is);
        if (G.overrun_bits || end > b.nbits) overruns += 1;
        requantize(T, ch, g, h.rate_idx, is, xr[ch]);
      }
      if (h.nch == 2) stereo(T, h, g, h.rate_idx, xr);
      for (int ch = 0; ch < h.nch; ++ch) {
        float sub[18][32];
        hybrid(T, ch, g, h.rate_idx, xr[ch], sub);
        float* dst = ch == 0 ? left->data() + base + 576 * g : (right ? right->data() + base + 576 * g : nullptr);
        float scratch[576];
        synth(T, ch, sub, dst ? dst : scratch);
      }
    }
    return 0;
  }
};

struct StreamInfo {
  int sample_rate = 0, channels = 0, bitrate_kbps = 0, vbr = 0;
  int frames = 0;              // audio frames decoded (a leading Xing / Info / VBRI frame is metadata and is not counted)
  int info_frames = 0;
  size_t id3v2_bytes = 0, junk_bytes = 0;  // junk: bytes skipped while searching for a frame header AFTER the first frame (sync losses)
  int resyncs = 0, overruns = 0, lost_reservoir = 0;
};

static size_t id3v2_size(const uint8_t* b, size_t len) {
  if (len < 10 || memcmp(b, "ID3", 3) || b[3] == 0xFF || b[4] == 0xFF || ((b[6] | b[7] | b[8] | b[9]) & 0x80)) return 0;
  const size_t sz = ((size_t)b[6] << 21) | ((size_t)b[7] << 14) | ((size_t)b[8] << 7) | b[9];
  return 10 + sz + ((b[5] & 0x10) ? 10 : 0);
}

// walks the frames; left == nullptr: headers and side information only
static int decode_stream(const uint8_t* b, size_t len, std::vector<float>* left, std::vector<float>* right, StreamInfo* info) {
  Decoder* dec = left ? new (std::nothrow) Decoder() : nullptr;
  if (left && !dec) return -1;
  size_t o = id3v2_size(b, len);
  info->id3v2_bytes = o;
  if (o > len) o = len;
  bool first = true;
  Header ref{};
  size_t junk_run = 0;
  while (o + 4 <= len) {
    Header h;
    bool ok = parse_header(b + o, &h) && o + (size_t)h.frame_bytes <= len + 0;
    if (ok && !first && (h.rate_idx != ref.rate_idx || h.nch != ref.nch)) ok = false;  // a stream does not change these mid-way
    if (ok && o + (size_t)h.frame_bytes + 4 <= len) {  // confirm with the next header where there is one
      Header n;
      const uint8_t* nx = b + o + h.frame_bytes;
      if (!(parse_header(nx, &n) && n.rate_idx == h.rate_idx && n.nch == h.nch) && memcmp(nx, "TAG", 3) != 0) ok = false;
    }
    if (!ok) {
      if (!memcmp(b + o, "TAG", 3) && len - o <= 128 + 227) break;  // ID3v1 (+ the enhanced tag) at the end of the file
      o += 1;
      junk_run += 1;
      continue;
    }
    if (junk_run) {
      if (!first) { info->junk_bytes += junk_run; info->resyncs += 1; }
      junk_run = 0;
    }
    if (first) {
      ref = h;
      info->sample_rate = kRate[h.rate_idx]; info->channels = h.nch; info->bitrate_kbps = h.bitrate;
      // a Xing / Info (LAME) or VBRI frame carries no audio: symphonia's reader consumes it as metadata
      const uint8_t* x = b + o + 4 + (h.crc ? 2 : 0) + h.side_bytes;
      const size_t room = (size_t)h.frame_bytes - (4 + (h.crc ? 2 : 0) + h.side_bytes);
      const bool xing = room >= 8 && (!memcmp(x, "Xing", 4) || !memcmp(x, "Info", 4));
      const bool vbri = h.frame_bytes >= 36 + 4 && !memcmp(b + o + 36, "VBRI", 4);
      first = false;
      if (xing || vbri) { info->info_frames += 1; o += h.frame_bytes; continue; }
    }
    if (h.bitrate != info->bitrate_kbps) info->vbr = 1;
    if (dec) {
      if (left->size() > ((size_t)1 << 28)) { delete dec; return -1; }  // > 1.7 h at 44.1 kHz in one body: refuse, stay bounded (1 GiB of f32)
      if (dec->decode_frame(b + o, h, left, right)) { delete dec; return -1; }
    }
    info->frames += 1;
    o += h.frame_bytes;
  }
  if (dec) { info->overruns = dec->overruns; info->lost_reservoir = dec->lost_reservoir; delete dec; }
  return info->frames > 0 ? 0 : -1;
}

// ---- resampler: the place of kaudio::resample (srv/batched_asr.rs:838) ----------------------------------------------------------
// Polyphase windowed-sinc interpolation for a rational ratio L / M (44.1 kHz -> 24 kHz: 80 / 147): output sample n sits at input
// position n M / L; the kernel is sinc(fc t) under a Kaiser window (beta 8.6: ~ -90 dB side lobes), 32 zero crossings each side,
// cut-off at 0.5 min(rate_in, rate_out) x 0.95.  kaudio is an un-vendored crate (it wraps a sinc resampler of the same family);
// its coefficients are not reproduced — parity unpinned, the properties are tested (DC gain, a tone keeps its frequency and
// level, images below -80 dB).
// The phase table (Kaiser beta 8.6, per-phase normalisation, stored as float) is dsm_pcm::phase_table (dsm_pcm_format.h), shared
// with the streaming per-slot ingest, whose definition is this function's output cut into frames.
static int resample(const float* in, size_t n, int rin, int rout, std::vector<float>* out) {
  if (rin <= 0 || rout <= 0) return -1;
  if (rin == rout) { out->assign(in, in + n); return 0; }
  long L = 0, M = 0;
  int half = 0;
  std::vector<float> ph;
  if (dsm_pcm::phase_table(rin, rout, &L, &M, &half, &ph)) return -1;
  const int taps = 2 * half;
  const size_t nout = (size_t)(((unsigned long long)n * (unsigned long long)L + M - 1) / M);
  out->resize(nout);
  for (size_t j = 0; j < nout; ++j) {
    const unsigned long long pos = (unsigned long long)j * M;
    const long i0 = (long)(pos / L), p = (long)(pos % L);
    const float* c = &ph[(size_t)p * taps];
    double a = 0.0;
    for (int k = 0; k < taps; ++k) {
      const long i = i0 + k - half + 1;
      if (i >= 0 && (size_t)i < n) a += (double)c[k] * in[i];
    }
    (*out)[j] = (float)a;
  }
  return 0;
}

}  // namespace dsm_mp3

extern "C" {

int dsm_mp3_probe(const uint8_t* bytes, size_t len, dsm_mp3_info* out) {
  if (!bytes || !out) return DSM_ERR_INVALID;
  dsm_mp3::StreamInfo si;
  memset(out, 0, sizeof *out);
  if (dsm_mp3::decode_stream(bytes, len, nullptr, nullptr, &si)) { g_create_error = "no MPEG-1 Layer III frame found"; return DSM_ERR_IO; }
  out->sample_rate = si.sample_rate; out->channels = si.channels; out->bitrate_kbps = si.bitrate_kbps; out->vbr = si.vbr;
  out->frames = si.frames; out->info_frames = si.info_frames; out->id3v2_bytes = (uint64_t)si.id3v2_bytes;
  out->junk_bytes = (uint64_t)si.junk_bytes; out->resyncs = si.resyncs;
  return 0;
}

static int mp3_decode_impl(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out, dsm_mp3_info* info) {
  if (!bytes || !pcm_out || !n_out) return DSM_ERR_INVALID;
  dsm_mp3::StreamInfo si;
  std::vector<float> left;
  if (dsm_mp3::decode_stream(bytes, len, &left, nullptr, &si)) { g_create_error = "no MPEG-1 Layer III frame found (MPEG-2 / 2.5 and Layers I / II are not decoded)"; return DSM_ERR_IO; }
  float* out = (float*)malloc(sizeof(float) * (left.size() ? left.size() : 1));
  if (!out) return DSM_ERR_IO;
  if (!left.empty()) memcpy(out, left.data(), sizeof(float) * left.size());
  *pcm_out = out; *n_out = left.size();
  if (sample_rate_out) *sample_rate_out = si.sample_rate;
  if (info) {
    memset(info, 0, sizeof *info);
    info->sample_rate = si.sample_rate; info->channels = si.channels; info->bitrate_kbps = si.bitrate_kbps; info->vbr = si.vbr;
    info->frames = si.frames; info->info_frames = si.info_frames; info->id3v2_bytes = (uint64_t)si.id3v2_bytes;
    info->junk_bytes = (uint64_t)si.junk_bytes; info->resyncs = si.resyncs; info->huffman_overruns = si.overruns;
    info->frames_without_reservoir = si.lost_reservoir;
  }
  return 0;
}

int dsm_mp3_decode(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out) {
  return mp3_decode_impl(bytes, len, pcm_out, n_out, sample_rate_out, nullptr);
}
int dsm_mp3_decode_info(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, dsm_mp3_info* info) {
  return mp3_decode_impl(bytes, len, pcm_out, n_out, nullptr, info);
}

int dsm_resample(const float* in, size_t n, int rate_in, int rate_out, float** out, size_t* n_out) {
  if ((!in && n) || !out || !n_out) return DSM_ERR_INVALID;
  std::vector<float> v;
  if (dsm_mp3::resample(in, n, rate_in, rate_out, &v)) { g_create_error = "unsupported resampling ratio"; return DSM_ERR_INVALID; }
  float* o = (float*)malloc(sizeof(float) * (v.size() ? v.size() : 1));
  if (!o) return DSM_ERR_IO;
  if (!v.empty()) memcpy(o, v.data(), sizeof(float) * v.size());
  *out = o; *n_out = v.size();
  return 0;
}

// srv/utils.rs:263-305 pcm_decode for the containers the reference's samples use: RIFF/WAVE or an MPEG-1 Layer III stream
int dsm_pcm_decode(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out) {
  if (!bytes || !pcm_out || !n_out) return DSM_ERR_INVALID;
  if (len >= 12 && !memcmp(bytes, "RIFF", 4)) return dsm_wav_decode(bytes, len, pcm_out, n_out, sample_rate_out);
  return dsm_mp3_decode(bytes, len, pcm_out, n_out, sample_rate_out);
}

// Test aids: the pieces of the filter bank on their own (tests/test_mp3.py pins them against their defining formulas)
int dsm_mp3_test_synth(const float* subbands /* [slots][32] */, int slots, float* pcm /* [slots * 32] */) {
  if (!subbands || !pcm || slots < 0) return DSM_ERR_INVALID;
  dsm_mp3::Decoder* d = new (std::nothrow) dsm_mp3::Decoder();
  if (!d) return DSM_ERR_IO;
  const dsm_mp3::Tables& T = dsm_mp3::tables();
  for (int s0 = 0; s0 < slots; s0 += 18) {
    float sub[18][32];
    memset(sub, 0, sizeof sub);
    const int ns = std::min(18, slots - s0);
    memcpy(sub, subbands + (size_t)s0 * 32, sizeof(float) * 32 * (size_t)ns);
    float out[576];
    d->synth(T, 0, sub, out);
    memcpy(pcm + (size_t)s0 * 32, out, sizeof(float) * 32 * (size_t)ns);
  }
  delete d;
  return 0;
}
int dsm_mp3_test_tables(int table, int* xlen, int* linbits, uint16_t* codes, uint8_t* lens, int cap) {
  if (table < 0 || table > 33 || !xlen || !linbits) return DSM_ERR_INVALID;
  const dsm_mp3::HuffDef& h = dsm_mp3::kHuff[table];
  *xlen = h.xlen; *linbits = h.linbits;
  const int n = h.code ? h.xlen * h.xlen : 0;
  for (int i = 0; i < n && i < cap; ++i) { if (codes) codes[i] = h.code[i]; if (lens) lens[i] = h.len[i]; }
  return n;
}
int dsm_mp3_test_imdct(const float* spectrum /* [18] */, int block_type, float* out /* [36] */) {
  if (!spectrum || !out || block_type < 0 || block_type > 3) return DSM_ERR_INVALID;
  const dsm_mp3::Tables& T = dsm_mp3::tables();
  for (int i = 0; i < 36; ++i) out[i] = 0.0f;
  if (block_type == 2) {
    for (int w = 0; w < 3; ++w)
      for (int i = 0; i < 12; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 6; ++k) s += spectrum[3 * k + w] * T.imdct_cos12[i][k];
        out[6 * w + 6 + i] += s * T.imdct_win[2][i];
      }
  } else {
    for (int i = 0; i < 36; ++i) {
      float s = 0.0f;
      for (int k = 0; k < 18; ++k) s += spectrum[k] * T.imdct_cos36[i][k];
      out[i] = s * T.imdct_win[block_type][i];
    }
  }
  return 0;
}

}  // extern "C"
