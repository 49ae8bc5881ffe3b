"""Every forward conv kernel, forced through the C ABI and asserted to be the kernel that ran, held to EQUALITY on integer operands
inside guard-banded buffers: the fp32 families behind w2l_conv_forward (implicit GEMM tiles with and without split-K, the split-operand
tiles, F(2x2) ids 6 / 7 / 8 / 9 / 12 / 19, F(4x4) id 11 in both packing forms, the fused-phase transposed kernels ids 10 / 20, the 7x7
first layer id 21, the direct 3x3 id 22), the bf16-storage families behind w2l_convb_forward (implicit GEMM tiles and split-K, stem,
box64, tp2b) and w2l_thin1x1_forward_bf16.  Cases, references and bounds: tests/_conv_cases.py (its docstring derives the bounds).

BUFFERS.  Every operand lives in the middle of a larger flat allocation [guard | tensor | guard]; a guard is
_conv_cases.guard_elems(cs): 512 pixels of the buffer's channel stride (conv_wino4 stores 32 tile slots x 16 pixels per work item,
the largest block any family stores; the bf16 implicit GEMM's largest tile is 256 rows), at least 64 KiB; the tensor's first element
stays 16-byte aligned.  OUTPUT: guards, neighbour channels and the tensor itself are pre-filled with a NaN that carries a payload;
after the launch guards and neighbour channels must be bit-identical to it and no element of the tensor may still hold it.  INPUTS
(x, res): guards and the channels outside the slice are NaN, the pad channels [cin, cin_p) zero as the ABI demands: a kernel that
lets a value from outside its tensor reach the result - even multiplied by a zero weight - turns the result into NaN.  Every address
handed to a kernel lies inside an allocation of the test; only the contents are hostile.

EXACT CHECK.  fp32 result == float64 reference; bf16-storage result == the reference rounded once to bf16; each case runs twice and
must be bit-identical.  ACCURACY CHECK.  One Gaussian run per family on the same buffers against float64: 1e-4 + 1e-4 |ref| (fp32),
|ref| / 128 + 2e-5 S (bf16); torch's own float32 convolution of the same operands is measured too - were it above a third of a
family's bound the bound would be three times its distance.  LARGE OFFSETS.  One exact case per launcher with x, y (and the residual)
between 1 GiB and the 2 GiB guard, data in the first and last image; just above 2 GiB the entry points refuse and leave y untouched.

`python tests/test_conv_exact_gpu.py` prints the selection table (on a GPU: with the kernel the launcher reports, after the bar; a
forced bf16 split-K is not reported by the launcher, those rows say what the test's own model of the K-steps gives):
  f32 igemm tile 0: ragged M and ragged cout                               conv 1->136 3x3 s1x1 p1 @13x11 N=3 id 0 | igemm 0
  f32 igemm tile 0: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 0 ks 3 | igemm 0 ks 3
  f32 igemm tile 1: ragged M and ragged cout                               conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 1 | igemm 1
  f32 igemm tile 1: split-K with a short last split                        convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 1 ks 3 | igemm 1 ks 3
  f32 igemm tile 2: ragged M and ragged cout                               conv 1->136 5x5 s1x2 p1 @13x11 N=3 id 2 | igemm 2
  f32 igemm tile 2: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 2 ks 3 | igemm 2 ks 3
  f32 igemm tile 3: ragged M and ragged cout                               conv 3->72 5x5 s1x2 p1 @13x11 N=3 id 3 | igemm 3
  f32 igemm tile 3: split-K with a short last split                        convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 3 ks 3 | igemm 3 ks 3
  f32 igemm tile 4: ragged M and ragged cout                               conv 6->40 5x5 s1x2 p1 @13x11 N=3 id 4 | igemm 4
  f32 igemm tile 4: split-K with a short last split                        convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 3 | igemm 4 ks 3
  f32 igemm tile 5: ragged M and ragged cout                               conv 1->136 3x3 s2x2 p1 @13x11 N=3 id 5 | igemm 5
  f32 igemm tile 5: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 5 ks 3 | igemm 5 ks 3
  f32 igemm: more splits asked than K-steps                                convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 64 | igemm 4 ks 10
  f32 igemm: split-K 3                                                     convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 3 | igemm 4 ks 3
  f32 igemm: cin_p > cin                                                   conv 1->72 1x1 s1x1 p0 @1x1 N=3 id 1 | igemm 1
  f32 igemm: transposed s1 p0                                              convT 1->40 3x3 s1x1 p0 @1x1 N=3 id 4 | igemm 4
  f32 igemm: transposed s2 p1 output padding 1, split-K                    convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 2 | igemm 4 ks 2
  f32 igemm: 7x7                                                           conv 6->16 7x7 s1x1 p3 @10x12 N=2 id 4 | igemm 4
  f32 igemm: 5x5 s(1,2)                                                    conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 1 | igemm 1
  f32 igemm: 3x3 s(3,2)                                                    conv 1->72 3x3 s3x2 p1 @9x6 N=3 id 3 | igemm 3
  f32 igemm: residual in its own buffer                                    conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 4 res | igemm 4
  f32 igemm: residual aliases the input                                    conv 64->64 3x3 s1x1 p1 @9x7 N=3 id 0 res=x | igemm 0
  f32 igemm: channel slices of wider buffers                               conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 4 res sliced | igemm 4
  f32 split tile 0: ragged M and ragged cout                               conv 1->136 3x3 s1x1 p1 @13x11 N=3 id 13 | split 13
  f32 split tile 0: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 13 ks 3 | split 13 ks 3
  f32 split tile 1: ragged M and ragged cout                               conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 14 | split 14
  f32 split tile 1: split-K with a short last split                        convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 14 ks 3 | split 14 ks 3
  f32 split tile 2: ragged M and ragged cout                               conv 1->136 5x5 s1x2 p1 @13x11 N=3 id 15 | split 15
  f32 split tile 2: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 15 ks 3 | split 15 ks 3
  f32 split tile 3: ragged M and ragged cout                               conv 3->72 5x5 s1x2 p1 @13x11 N=3 id 16 | split 16
  f32 split tile 3: split-K with a short last split                        convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 16 ks 3 | split 16 ks 3
  f32 split tile 4: ragged M and ragged cout                               conv 6->40 5x5 s1x2 p1 @13x11 N=3 id 17 | split 17
  f32 split tile 4: split-K with a short last split                        convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 17 ks 3 | split 17 ks 3
  f32 split tile 5: ragged M and ragged cout                               conv 1->136 3x3 s2x2 p1 @13x11 N=3 id 18 | split 18
  f32 split tile 5: split-K with a short last split                        convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 18 ks 3 | split 18 ks 3
  f32 split: more splits asked than K-steps                                convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 17 ks 64 | split 17 ks 10
  f32 split: split-K 3                                                     convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 17 ks 3 | split 17 ks 3
  f32 split: cin_p > cin                                                   conv 1->72 1x1 s1x1 p0 @1x1 N=3 id 14 | split 14
  f32 split: transposed s1 p0                                              convT 1->40 3x3 s1x1 p0 @1x1 N=3 id 17 | split 17
  f32 split: transposed s2 p1 output padding 1, split-K                    convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 17 ks 2 | split 17 ks 2
  f32 split: 7x7                                                           conv 6->16 7x7 s1x1 p3 @10x12 N=2 id 17 | split 17
  f32 split: 5x5 s(1,2)                                                    conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 14 | split 14
  f32 split: 3x3 s(3,2)                                                    conv 1->72 3x3 s3x2 p1 @9x6 N=3 id 16 | split 16
  f32 split: residual in its own buffer                                    conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 17 res | split 17
  f32 split: residual aliases the input                                    conv 64->64 3x3 s1x1 p1 @9x7 N=3 id 13 res=x | split 13
  f32 split: channel slices of wider buffers                               conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 17 res sliced | split 17
  bf16 igemm tile 0: ragged M and ragged cout                              conv 1->136 3x3 s1x1 p1 @13x11 N=3 id 0 | igemm 0
  bf16 igemm tile 0: split-K with a short last split                       convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 0 ks 2 | igemm 0 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm tile 1: ragged M and ragged cout                              conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 1 | igemm 1
  bf16 igemm tile 1: split-K with a short last split                       convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 1 ks 2 | igemm 1 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm tile 2: ragged M and ragged cout                              conv 1->136 5x5 s1x2 p1 @13x11 N=3 id 2 | igemm 2
  bf16 igemm tile 2: split-K with a short last split                       convT 80->136 3x3 s2x2 p1+1 @5x3 N=2 id 2 ks 2 | igemm 2 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm tile 3: ragged M and ragged cout                              conv 3->72 5x5 s1x2 p1 @13x11 N=3 id 3 | igemm 3
  bf16 igemm tile 3: split-K with a short last split                       convT 80->72 3x3 s2x2 p1+1 @5x3 N=2 id 3 ks 2 | igemm 3 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm tile 4: ragged M and ragged cout                              conv 6->40 5x5 s1x2 p1 @13x11 N=3 id 4 | igemm 4
  bf16 igemm tile 4: split-K with a short last split                       convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 2 | igemm 4 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm tile 5: ragged M and ragged cout                              conv 80->264 3x3 s1x1 p1 @13x11 N=3 id 5 | igemm 5
  bf16 igemm tile 5: split-K with a short last split                       conv 64->64 3x3 s1x1 p1 @9x7 N=2 id 5 ks 2 res=x sliced | igemm 5 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm: more splits asked than K-steps                               convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 64 | igemm 4 (forced split-K 64: 5 splits by the test's own model, unchecked)
  bf16 igemm: split-K 3                                                    convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 3 | igemm 4 (forced split-K 3: 3 splits by the test's own model, unchecked)
  bf16 igemm: cin_p > cin                                                  conv 1->72 1x1 s1x1 p0 @1x1 N=3 id 1 | igemm 1
  bf16 igemm: transposed s1 p0                                             convT 1->40 3x3 s1x1 p0 @1x1 N=3 id 4 | igemm 4
  bf16 igemm: transposed s2 p1 output padding 1, split-K                   convT 80->40 3x3 s2x2 p1+1 @5x3 N=2 id 4 ks 2 | igemm 4 (forced split-K 2: 2 splits by the test's own model, unchecked)
  bf16 igemm: 7x7                                                          conv 1->136 7x7 s1x1 p3 @13x11 N=3 id 0 | igemm 0
  bf16 igemm: 5x5 s(1,2)                                                   conv 1->72 5x5 s1x2 p2 @13x11 N=3 id 1 | igemm 1
  bf16 igemm: 3x3 s(3,2)                                                   conv 1->72 3x3 s3x2 p1 @9x6 N=3 id 3 | igemm 3
  bf16 igemm: residual in its own buffer                                   conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 4 res | igemm 4
  bf16 igemm: residual aliases the input                                   conv 64->64 3x3 s1x1 p1 @9x7 N=3 id 0 res=x | igemm 0
  bf16 igemm: channel slices of wider buffers                              conv 15->40 3x3 s1x1 p1 @9x7 N=3 id 4 res sliced | igemm 4
  wino id 6: a single pixel                                                conv 8->64 3x3 s1x1 p1 @1x1 N=1 id 6 | wino 6
  wino id 6: odd extents, several tiles                                    conv 8->64 3x3 s1x1 p1 @13x11 N=1 id 6 | wino 6
  wino id 6: residual in its own buffer                                    conv 8->64 3x3 s1x1 p1 @5x4 N=3 id 6 res | wino 6
  wino id 6: residual aliases the input                                    conv 64->64 3x3 s1x1 p1 @5x4 N=3 id 6 res=x | wino 6
  wino id 6: channel slices of wider buffers                               conv 8->64 3x3 s1x1 p1 @13x11 N=3 id 6 res sliced | wino 6
  wino id 7: a single pixel                                                conv 16->128 3x3 s1x1 p1 @1x1 N=1 id 7 | wino 7
  wino id 7: odd extents, several tiles                                    conv 16->128 3x3 s1x1 p1 @13x11 N=1 id 7 | wino 7
  wino id 7: residual in its own buffer                                    conv 16->128 3x3 s1x1 p1 @5x4 N=3 id 7 res | wino 7
  wino id 7: residual aliases the input                                    conv 128->128 3x3 s1x1 p1 @5x4 N=3 id 7 res=x | wino 7
  wino id 7: channel slices of wider buffers                               conv 16->128 3x3 s1x1 p1 @13x11 N=3 id 7 res sliced | wino 7
  wino id 8: a single pixel                                                conv 8->64 3x3 s1x1 p1 @1x1 N=1 id 8 | wino2 8
  wino id 8: odd extents, several tiles                                    conv 8->64 3x3 s1x1 p1 @13x11 N=1 id 8 | wino2 8
  wino id 8: residual in its own buffer                                    conv 8->64 3x3 s1x1 p1 @5x4 N=3 id 8 res | wino2 8
  wino id 8: residual aliases the input                                    conv 64->64 3x3 s1x1 p1 @5x4 N=3 id 8 res=x | wino2 8
  wino id 8: channel slices of wider buffers                               conv 8->64 3x3 s1x1 p1 @13x11 N=3 id 8 res sliced | wino2 8
  wino id 9: a single pixel                                                conv 8->32 3x3 s1x1 p1 @1x1 N=1 id 9 | wino2 9
  wino id 9: odd extents, several tiles                                    conv 8->32 3x3 s1x1 p1 @13x11 N=1 id 9 | wino2 9
  wino id 9: residual in its own buffer                                    conv 8->32 3x3 s1x1 p1 @5x4 N=3 id 9 res | wino2 9
  wino id 9: residual aliases the input                                    conv 32->32 3x3 s1x1 p1 @5x4 N=3 id 9 res=x | wino2 9
  wino id 9: channel slices of wider buffers                               conv 32->32 3x3 s1x1 p1 @5x4 N=3 id 9 res=x sliced | wino2 9
  wino id 12: a single pixel                                               conv 8->32 3x3 s1x1 p1 @1x1 N=1 id 12 | wino2 12
  wino id 12: odd extents, several tiles                                   conv 8->32 3x3 s1x1 p1 @13x11 N=1 id 12 | wino2 12
  wino id 12: residual in its own buffer                                   conv 8->32 3x3 s1x1 p1 @5x4 N=3 id 12 res | wino2 12
  wino id 12: residual aliases the input                                   conv 32->32 3x3 s1x1 p1 @5x4 N=3 id 12 res=x | wino2 12
  wino id 12: channel slices of wider buffers                              conv 32->32 3x3 s1x1 p1 @5x4 N=3 id 12 res=x sliced | wino2 12
  wino id 11: a single pixel                                               conv 8->64 3x3 s1x1 p1 @1x1 N=1 id 11 | wino4 11
  wino id 11: odd extents, several tiles                                   conv 8->64 3x3 s1x1 p1 @13x11 N=1 id 11 | wino4 11
  wino id 11: residual in its own buffer                                   conv 8->64 3x3 s1x1 p1 @5x4 N=3 id 11 res | wino4 11
  wino id 11: residual aliases the input                                   conv 64->64 3x3 s1x1 p1 @5x4 N=3 id 11 res=x | wino4 11
  wino id 11: channel slices of wider buffers                              conv 8->64 3x3 s1x1 p1 @13x11 N=3 id 11 res sliced | wino4 11
  wino id 19: a single pixel                                               conv 16->64 3x3 s1x1 p1 @1x1 N=1 id 19 | wino2s 19
  wino id 19: odd extents, several tiles                                   conv 16->64 3x3 s1x1 p1 @13x11 N=1 id 19 | wino2s 19
  wino id 19: residual in its own buffer                                   conv 16->64 3x3 s1x1 p1 @5x4 N=3 id 19 res | wino2s 19
  wino id 19: residual aliases the input                                   conv 64->64 3x3 s1x1 p1 @5x4 N=3 id 19 res=x | wino2s 19
  wino id 19: channel slices of wider buffers                              conv 64->64 3x3 s1x1 p1 @5x4 N=3 id 19 res=x sliced | wino2s 19
  wino id 8: several images per block, last group past the batch           conv 8->64 3x3 s1x1 p1 @1x1 N=5 id 8 | wino2 8
  wino id 8: the same with several tiles per image                         conv 8->64 3x3 s1x1 p1 @3x3 N=5 id 8 | wino2 8
  wino id 9: several images per block, last group past the batch           conv 8->32 3x3 s1x1 p1 @1x1 N=3 id 9 | wino2 9
  wino id 9: the same with several tiles per image                         conv 8->32 3x3 s1x1 p1 @3x3 N=3 id 9 | wino2 9
  wino id 12: several images per block, last group past the batch          conv 8->32 3x3 s1x1 p1 @1x1 N=5 id 12 | wino2 12
  wino id 12: the same with several tiles per image                        conv 8->32 3x3 s1x1 p1 @3x3 N=5 id 12 | wino2 12
  wino id 19: several images per block, last group past the batch          conv 16->64 3x3 s1x1 p1 @1x1 N=5 id 19 | wino2s 19
  wino id 19: the same with several tiles per image                        conv 16->64 3x3 s1x1 p1 @3x3 N=5 id 19 | wino2s 19
  wino4: rectangles                                                        conv 8->64 3x3 s1x1 p1 @1x1 N=1 id 11 | wino4 11
  wino4: rectangles, several images per block, last group past the batch   conv 8->64 3x3 s1x1 p1 @1x1 N=5 id 11 | wino4 11
  wino4: segments                                                          conv 8->64 3x3 s1x1 p1 @13x11 N=5 id 11 | wino4 11
  wino4: segments, a block starts in the middle of an image                conv 8->64 3x3 s1x1 p1 @13x11 N=5 id 11 | wino4 11
  wino4: segments, a block covers three images                             conv 8->64 3x3 s1x1 p1 @13x11 N=5 id 11 | wino4 11
  wino4: segments, the last block is short                                 conv 8->64 3x3 s1x1 p1 @13x11 N=7 id 11 | wino4 11
  tp2: a single input pixel                                                convT 16->128 3x3 s2x2 p1+1 @1x1 N=1 id 10 | tp2 10
  tp2: odd extents, odd batch                                              convT 8->64 3x3 s2x2 p1+1 @5x7 N=7 id 10 | tp2 10
  tp2: channel slices of wider buffers                                     convT 64->64 3x3 s2x2 p1+1 @9x16 N=3 id 10 sliced | tp2 10
  tp2s: a single input pixel                                               convT 16->128 3x3 s2x2 p1+1 @1x1 N=1 id 20 | tp2s 20
  tp2s: odd extents, odd batch                                             convT 16->64 3x3 s2x2 p1+1 @5x7 N=7 id 20 | tp2s 20
  tp2s: channel slices of wider buffers                                    convT 64->64 3x3 s2x2 p1+1 @9x16 N=3 id 20 sliced | tp2s 20
  tp2: several images per block, last group past the batch                 convT 16->128 3x3 s2x2 p1+1 @1x1 N=7 id 10 | tp2 10
  tp2: the same with several pixels per image                              convT 8->64 3x3 s2x2 p1+1 @5x7 N=3 id 10 | tp2 10
  tp2s: several images per block, last group past the batch                convT 16->128 3x3 s2x2 p1+1 @1x1 N=7 id 20 | tp2s 20
  tp2s: the same with several pixels per image                             convT 16->64 3x3 s2x2 p1+1 @5x7 N=3 id 20 | tp2s 20
  k3s: several images per block, last group past the batch                 conv 16->32 3x3 s1x1 p1 @1x1 N=5 id 22 | k3s 22
  k3s: the same with several pixels per image                              conv 16->32 3x3 s1x1 p1 @5x7 N=5 id 22 | k3s 22
  tp2s: split-K 2                                                          convT 64->64 3x3 s2x2 p1+1 @9x16 N=1 id 20 ks 2 | tp2s 20 ks 2
  tp2s: split-K 3 with a short last split                                  convT 80->64 3x3 s2x2 p1+1 @3x2 N=2 id 20 ks 3 | tp2s 20 ks 3
  tp2s: more splits asked than K-steps                                     convT 16->128 3x3 s2x2 p1+1 @1x1 N=1 id 20 ks 2 | tp2s 20
  stem7s: image smaller than a block                                       conv 5->16 7x7 s1x1 p3 @5x3 N=1 id 21 | stem7s 21
  stem7s: ragged blocks in both directions                                 conv 5->16 7x7 s1x1 p3 @50x37 N=1 id 21 | stem7s 21
  stem7s: 5 input channels (cin_p > cin)                                   conv 5->16 7x7 s1x1 p3 @5x3 N=1 id 21 | stem7s 21
  stem7s: channel slices of wider buffers                                  conv 6->16 7x7 s1x1 p3 @16x16 N=2 id 21 sliced | stem7s 21
  k3s: a single pixel                                                      conv 16->32 3x3 s1x1 p1 @1x1 N=1 id 22 | k3s 22
  k3s: five K-steps                                                        conv 80->32 3x3 s1x1 p1 @1x1 N=1 id 22 | k3s 22
  k3s: residual in its own buffer                                          conv 16->32 3x3 s1x1 p1 @5x7 N=3 id 22 res | k3s 22
  k3s: residual aliases the input                                          conv 32->32 3x3 s1x1 p1 @5x7 N=3 id 22 res=x | k3s 22
  k3s: channel slices of wider buffers                                     conv 32->32 3x3 s1x1 p1 @5x7 N=3 id 22 res=x sliced | k3s 22
  bf16 stem: 7x7, cin_p 8                                                  conv 3->16 7x7 s1x1 p3 @16x16 N=1024 | stem1
  bf16 stem: 7x7, cin_p 16                                                 conv 15->16 7x7 s1x1 p3 @16x16 N=1024 | stem1
  bf16 stem: 80 -> 32 output block                                         conv 80->32 3x3 s1x1 p1 @16x16 N=2048 | stem2
  bf16 stem: 32 -> 32 with a residual                                      conv 32->32 3x3 s1x1 p1 @16x16 N=2048 res | stem3
  bf16 stem: tiles not a multiple of the grid                              conv 3->16 7x7 s1x1 p3 @16x16 N=1030 | stem1
  bf16 stem: channel slices of wider buffers                               conv 6->16 7x7 s1x1 p3 @16x16 N=1030 sliced | stem1
  bf16 box64: no residual                                                  conv 64->64 3x3 s1x1 p1 @16x16 N=2048 | box64
  bf16 box64: residual aliases the input                                   conv 64->64 3x3 s1x1 p1 @16x16 N=2048 res=x | box64
  bf16 box64: ragged tiles, 60 couts, slices                               conv 64->60 3x3 s1x1 p1 @15x15 N=2048 res sliced | box64
  bf16 tp2b: odd extents                                                   convT 32->32 3x3 s2x2 p1+1 @5x7 N=2049 | tp2b
  bf16 tp2b: a single input pixel                                          convT 64->24 3x3 s2x2 p1+1 @1x1 N=2049 | tp2b
  bf16 tp2b: channel slices of wider buffers                               convT 32->32 3x3 s2x2 p1+1 @5x7 N=1030 sliced | tp2b
  head without activation: igemm                                           conv 15->32 3x3 s1x1 p1 @9x7 N=3 id 0 head 3 | igemm 0
  head without activation: split                                           conv 15->32 3x3 s1x1 p1 @9x7 N=3 id 13 head 3 | split 13
  head without activation: k3s                                             conv 48->32 3x3 s1x1 p1 @1x1 N=9 id 22 head 1 | k3s 22
  head without activation: k3s_head                                        conv 48->32 3x3 s1x1 p1 @1x1 N=9 head 1 | k3s_head
  head without activation: wino2 id 9                                      conv 8->32 3x3 s1x1 p1 @13x11 N=3 id 9 head 3 | wino2 9
  head without activation: wino2 id 12                                     conv 8->32 3x3 s1x1 p1 @13x11 N=3 id 12 head 3 | wino2 12
  head without activation: output slice of a wider pixel                   conv 8->32 3x3 s1x1 p1 @5x4 N=3 id 9 head 3 sliced | wino2 9
  thin: one pixel                                                          conv 5->1 1x1 s1x1 p0 @1x1 N=1 | thin
  thin: several blocks, ragged tail                                        conv 5->1 1x1 s1x1 p0 @1x777 N=1 | thin
  thin: cin not a multiple of 8                                            conv 5->1 1x1 s1x1 p0 @1x1 N=1 | thin
  thin: channel slices of wider buffers                                    conv 32->3 1x1 s1x1 p0 @1x777 N=1 sliced | thin
  large offsets: f32/igemm conv 8->72 3x3 s1x1 p1 @12x12 N=4096 id 3 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/igemm conv 8->72 3x3 s2x2 p1 @12x12 N=4096 id 1 ks 2 cs 2048 x 1.12 GiB  y 1.12 GiB  res 0.00 GiB
  large offsets: f32/split conv 8->72 3x3 s1x1 p1 @12x12 N=4096 id 16 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino conv 8->64 3x3 s1x1 p1 @12x12 N=4096 id 6 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino conv 16->128 3x3 s1x1 p1 @12x12 N=4096 id 7 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino2 conv 8->64 3x3 s1x1 p1 @12x12 N=4096 id 8 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino2 conv 8->32 3x3 s1x1 p1 @12x12 N=4096 id 9 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino2 conv 8->32 3x3 s1x1 p1 @12x12 N=4096 id 12 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino4 conv 8->64 3x3 s1x1 p1 @12x12 N=4096 id 11 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/wino2s conv 16->64 3x3 s1x1 p1 @12x12 N=4096 id 19 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: f32/tp2 convT 8->64 3x3 s2x2 p1+1 @5x7 N=16384 id 10 cs 128 x 1.09 GiB  y 1.09 GiB  res 0.00 GiB
  large offsets: f32/tp2s convT 16->64 3x3 s2x2 p1+1 @5x7 N=16384 id 20 cs 128 x 1.09 GiB  y 1.09 GiB  res 0.00 GiB
  large offsets: f32/tp2s convT 32->64 3x3 s2x2 p1+1 @5x7 N=16384 id 20 ks 2 cs 128 x 1.09 GiB  y 1.09 GiB  res 0.00 GiB
  large offsets: f32/stem7s conv 6->16 7x7 s1x1 p3 @12x12 N=4096 id 21 cs 512 x 1.12 GiB  y 1.12 GiB  res 0.00 GiB
  large offsets: f32/k3s conv 16->32 3x3 s1x1 p1 @12x12 N=4096 id 22 res cs 512 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: bf16/igemm conv 8->72 3x3 s1x1 p1 @12x12 N=4096 id 3 res cs 1024 x 1.12 GiB  y 1.12 GiB  res 1.12 GiB
  large offsets: bf16/igemm conv 8->72 3x3 s1x1 p1 @12x12 N=4096 id 1 ks 2 cs 1024 x 1.12 GiB  y 1.12 GiB  res 0.00 GiB
  large offsets: bf16/stem conv 6->16 7x7 s1x1 p3 @16x16 N=4200 cs 512   x 1.03 GiB  y 1.03 GiB  res 0.00 GiB
  large offsets: bf16/box64 conv 64->64 3x3 s1x1 p1 @16x16 N=4200 res cs 512 x 1.03 GiB  y 1.03 GiB  res 1.03 GiB
  large offsets: bf16/tp2b convT 32->32 3x3 s2x2 p1+1 @5x7 N=16384 cs 256 x 1.09 GiB  y 1.09 GiB  res 0.00 GiB
  large offsets: thin/thin conv 32->3 1x1 s1x1 p0 @1x1000 N=600 cs 1024  x 1.14 GiB  y 1.14 GiB  res 0.00 GiB
"""
import ctypes as C

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file runs as a script)
import _conv_cases as cc
from wav2lip_amd import _lib, bf16
from wav2lip_amd._lib import check, current_stream

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC0DEAD          # fp32 NaN with a payload
SENT16 = 0x7FD5              # bf16 NaN with a payload
_FAULTED = []                # a HIP error from a synchronisation: nothing more is launched by this module


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError:
        _FAULTED.append(1)
        raise


class Buf:
    """[guard | N x H x W x cs | guard]; the slice is channels [off, off + cw) of every pixel"""

    def __init__(self, case, N, H, W, cs, off, cw, device, out, f32=False):
        self.dtype = torch.float32 if case.path == "f32" or f32 else torch.bfloat16
        self.esz = 4 if self.dtype == torch.float32 else 2
        self.shape, self.cs, self.off, self.cw, self.out = (N, H, W), cs, off, cw, out
        self.g = cc.guard_elems(cs, self.esz)
        self.n = N * H * W * cs
        self.flat = torch.empty(2 * self.g + self.n, dtype=self.dtype, device=device)
        self.bits = self.flat.view(torch.int32 if self.esz == 4 else torch.int16)
        self.sent = SENT32 if self.esz == 4 else SENT16
        self.body = self.flat[self.g:self.g + self.n].view(N, H, W, cs)
        self.bbits = self.bits[self.g:self.g + self.n].view(N, H, W, cs)
        assert self.body.data_ptr() % 16 == 0 and (off * self.esz) % 16 == 0 and off + cw <= cs
        self.reset()

    def reset(self):
        if self.out:
            self.bits.fill_(self.sent)
        else:
            self.flat.fill_(float("nan"))

    @property
    def ptr(self):
        return C.c_void_p(self.body.data_ptr() + self.off * self.esz)

    def load(self, stack, imap):
        """stack [D, C, H, W] float64 (host) -> channels [off, off + cw) of every image (pad channels zero)"""
        D, Cn = stack.shape[:2]
        t = torch.zeros((D,) + self.shape[1:] + (self.cw,), dtype=torch.float64)
        t[..., :Cn] = stack.permute(0, 2, 3, 1)
        t = t.to(self.dtype).to(self.flat.device)
        if imap == list(range(D)):
            self.body[..., self.off:self.off + self.cw] = t
        else:
            self.body[..., self.off:self.off + self.cw] = t[torch.tensor(imap, device=t.device)]

    def written(self):
        return self.bbits[..., self.off:self.off + self.cw].clone()

    def check_untouched(self, what):
        s = self.sent
        assert bool((self.bits[:self.g] == s).all()), "%s: wrote before the first pixel" % what
        assert bool((self.bits[self.g + self.n:] == s).all()), "%s: wrote after the last pixel" % what
        assert bool((self.bbits[..., :self.off] == s).all()) and bool((self.bbits[..., self.off + self.cw:] == s).all()), \
            "%s: wrote into the neighbour channels" % what
        left = int((self.bbits[..., self.off:self.off + self.cw] == s).sum())
        assert left == 0, "%s: %d elements of the tensor were never written" % (what, left)


def _launcher(case, w, scale, shift, device):
    """(run(x, y, res), ran): run enqueues one launch; ran = (family, id / tile, split-K, executed FLOPs or None) of the kernel that
    runs, from the launcher itself; the objects that own device memory stay alive in the closure"""
    lib = _lib.load()
    wd = w.float().contiguous().to(device)
    sc, sh = scale.float().contiguous().to(device), shift.float().contiguous().to(device)
    N, H, W = case.N, case.H, case.W
    if case.path == "thin":
        wd = wd.view(case.cout, case.cin).contiguous()

        def run(x, y, res):
            check(lib.w2l_thin1x1_forward_bf16(current_stream(), N * H * W, case.cin, case.cout, x.ptr, x.cs, _lib.ptr(wd), _lib.ptr(sh),
                                               case.act, y.ptr, y.cs), "thin1x1_forward")
        return run, lambda x, y, res: ("thin", -1, 1, None)
    if case.path == "bf16" and case.head:
        layer = bf16.ConvB(case.geom(), wd)
        hw, hb = (t.float().contiguous().to(device) for t in cc.head_operands(case))
        check(lib.w2l_convb_attach_head(layer.handle, _lib.ptr(wd), _lib.ptr(hw), _lib.ptr(hb), case.head, cc.ACT_NONE,
                                        current_stream()), "convb_attach_head")
        gf = cc.GUARD_MIN_BYTES  # guard bytes on either side of the uint8 frames
        frames = torch.full((2 * gf + N * H * W * case.head,), 0xA5, dtype=torch.uint8, device=device)

        aff = {"sc": sc, "sh": sh}      # a bf16 launch takes scale / shift per call: the update test swaps them here

        def run(x, y, res, _keep=(hw, hb)):
            frames.fill_(0xA5)
            check(lib.w2l_convb_forward_head(layer.handle, current_stream(), N, H, W, x.ptr, x.cs, C.c_void_p(frames.data_ptr() + gf),
                                             y.ptr, y.cs, _lib.ptr(aff["sc"]), _lib.ptr(aff["sh"])), "convb_forward_head")
        run.frames, run.gf, run.layer, run.aff = frames, gf, layer, aff
        return run, lambda x, y, res: layer.resolve(N, H, W) + (None,)
    if case.path == "bf16":
        layer = bf16.ConvB(case.geom(), wd)
        if case.force >= 0:
            layer.set_tile(case.force)
        aff = {"sc": sc, "sh": sh}

        def run(x, y, res):
            check(lib.w2l_convb_forward(layer.handle, current_stream(), N, H, W, x.ptr, x.cs, y.ptr, y.cs, res.ptr if res else None,
                                        res.cs if res else 0, _lib.ptr(aff["sc"]), _lib.ptr(aff["sh"]), case.ks), "convb_forward")
        run.layer, run.aff = layer, aff

        def ran(x, y, res):      # w2l_convb_resolve answers for ksplit_force 0: a forced split-K is not reported by the launcher
            fam, tile, ks = layer.resolve(N, H, W, res=bool(case.res))
            return (fam, tile, ks, None)
        return run, ran
    g = case.geom()
    h, p = C.c_void_p(), C.c_void_p()
    check(lib.w2l_conv_create(C.byref(g), _lib.ptr(wd), _lib.ptr(sc), _lib.ptr(sh), current_stream(), C.byref(h)), "conv_create")
    if case.head:
        hw, hb = (t.float().contiguous().to(device) for t in cc.head_operands(case))
        check(lib.w2l_conv_attach_head(h, _lib.ptr(hw), _lib.ptr(hb), case.head, cc.ACT_NONE, current_stream()), "conv_attach_head")
    check(lib.w2l_plan_create(C.byref(p)), "plan_create")
    state = {"added": False}

    class Owner:
        def __del__(self):
            lib.w2l_plan_destroy(p)
            lib.w2l_conv_destroy(h)
    owner = Owner()

    def add(x, y, res):
        if not state["added"]:
            check(lib.w2l_plan_add_conv(p, h, N, H, W, x.ptr, x.cs, y.ptr, y.cs, res.ptr if res else None, res.cs if res else 0),
                  "plan_add_conv")
            check(lib.w2l_plan_set_config(p, 0, case.force, case.ks or 1), "plan_set_config")
            state["added"] = True

    def run(x, y, res, _o=owner):
        add(x, y, res)
        check(lib.w2l_plan_run(p, current_stream()), "plan_run")
    run.handle = h

    def ran(x, y, res):
        add(x, y, res)
        fl, cfg = (C.c_longlong * 1)(), (C.c_int * 2)()
        check(lib.w2l_plan_executed_flops(p, fl, cfg), "plan_executed_flops")
        return (_lib.FAMILY_NAMES[lib.w2l_conv_config_family(cfg[0])], int(cfg[0]), int(cfg[1]), int(fl[0]))
    return run, ran


def _assert_ran(case, ran):
    """the forced kernel is the one that runs (an ineligible id falls back silently and must not count)"""
    fam, cid, ks, flops = ran
    if case.path == "thin":
        return
    if case.path == "bf16":
        if case.head:
            assert fam == "k3s_head", (case, ran)
        elif case.force >= 0:
            assert (fam, cid) == ("igemm", case.force), (case, ran)
        else:
            assert fam.startswith(case.family), (case, ran)
        return
    assert fam == case.family and cid == case.force, (case, ran)
    if case.family in ("igemm", "split") and not case.head:
        assert ks == case.splits()[0] or (case.cout <= 16 and ks == 1), (case, ran, case.splits())
        if case.cout > 16:     # the tile table of _conv_cases against the launcher's padded-tile FLOP count
            bm, bn = case.tile()
            cout_p = (case.cout + 31) // 32 * 32
            tiles = -(-case.gemm_rows() // bm) * bm * -(-cout_p // bn) * bn
            per = 2 * tiles * (6 if case.family == "split" else 1)
            if case.tr:     # several phases of different depth: the padded tiles divide the count
                assert flops % per == 0, (case, ran, tiles)
            else:
                assert flops == per * case.ksteps() * cc.KSTEP["f32"], (case, ran, tiles)
    elif case.family == "tp2s":
        steps = case.cin // 16
        want = max(1, min(case.ks or 1, steps))
        assert ks == -(-steps // -(-steps // want)), (case, ran)


def _buffers(case, device):
    ho, wo = case.out_hw()
    xs, xo, ys, yo, rs, ro = case.strides()
    x = Buf(case, case.N, case.H, case.W, xs, xo, case.cin_p, device, out=False)
    y = Buf(case, case.N, ho, wo, ys, yo, case.cout_w, device, out=True, f32=bool(case.head))
    res = None
    if case.res == 1:
        res = Buf(case, case.N, ho, wo, rs, ro, case.cout_w, device, out=False)
    elif case.res == 2:
        res = x
    elif case.res == 3:      # an accumulating launch: the residual IS the output slice (test_conv_backward_exact_gpu.py)
        res = y
    return x, y, res


def _expected(case, ref, imap, device):
    """ref [D, cout, Ho, Wo] float64 -> [N, Ho, Wo, cout_w] in the storage type (bf16: ONE rounding; pad channels zero)"""
    D = ref.shape[0]
    t = torch.zeros((D,) + tuple(ref.shape[2:]) + (case.cout_w,), dtype=torch.float64)
    t[..., :ref.shape[1]] = ref.permute(0, 2, 3, 1)
    if case.path == "f32" or case.head:
        assert bool((t.float().double() == t).all())
        t = t.float()
    else:
        t = t.float().bfloat16()             # exact in fp32 (the bound), then one RNE rounding
    return t.to(device)[torch.tensor(imap, device=device)]


def _load_prior(case, y, res64, imap):
    """res = 3: the output slice holds the prior gradient before every launch (pad channels zero); everything around it the sentinel"""
    if case.res == 3:
        y.load(res64, imap)


def _compare(case, y, want, what):
    """guards and neighbour channels untouched, every element written, the slice equal to `want`"""
    y.check_untouched(what)
    got = y.body[..., y.off:y.off + y.cw]
    bad = int((got != want).sum())            # NaN != anything: a poisoned element counts
    assert bad == 0, "%s: %d of %d elements differ from the float64 reference; first at %s" % (
        what, bad, want.numel(), (got != want).nonzero()[0].tolist())


def run_exact(case, device):
    assert not _FAULTED, "an earlier case ended in a HIP error: nothing more is launched"
    assert cc.eligible(case), case
    assert case.exact_bound() < cc.LIMIT, (case, case.exact_bound())
    x64, w64, scale, shift, res64 = cc.int_operands(case)
    ref = cc.ref64(case, x64, w64, scale, shift, res64)
    if case.head:
        ref = cc.head_ref(ref, *cc.head_operands(case))
    D, imap = cc.image_map(case)
    assert float(ref[:2].abs().max()) > 0
    x, y, res = _buffers(case, device)
    x.load(x64, imap)
    if case.res == 1:
        res.load(res64, imap)
    _load_prior(case, y, res64, imap)
    run, ran = _launcher(case, w64, scale, shift, device)
    got_ran = ran(x, y, res)
    _assert_ran(case, got_ran)
    run(x, y, res)
    _sync()
    first = y.written()
    want = _expected(case, ref, imap, device)
    _compare(case, y, want, repr(case))
    if case.head and case.path == "bf16":      # the uint8 frames: (uint8)(int)(v * 255.f) of the same values, nothing around them
        fr = run.frames[run.gf:-run.gf].view(want.shape).long()
        assert torch.equal(fr, (want * 255.0).trunc().long() % 256), "%r: uint8 frames differ" % (case,)
        assert bool((run.frames[:run.gf] == 0xA5).all()) and bool((run.frames[-run.gf:] == 0xA5).all()), "%r: wrote around the frames" % (case,)
    y.reset()
    _load_prior(case, y, res64, imap)
    run(x, y, res)
    _sync()
    y.check_untouched(repr(case) + " (second run)")
    assert torch.equal(first, y.written()), "%r: two runs differ" % (case,)
    return got_ran


def _pool_params():
    out = []
    for pool in cc.POOLS:
        out += [pytest.param(c, id=pool.replace(" ", "_") + "-" + c.describe().replace(" ", "_")) for c in cc.exact_cases(pool)]
    return out


@pytest.mark.parametrize("case", _pool_params())
def test_exact(case, cuda):
    """every eligible candidate of every family: equality with float64, guard bands, neighbour channels, two identical runs"""
    run_exact(case, cuda)


@pytest.mark.parametrize("name", [n for n, _p, _c in cc.REGIMES])
def test_regime(name, cuda):
    """the case the selection gives a regime satisfies the regime's predicate (from the planning functions) and runs exactly on the
    kernel it names"""
    sel = {n: c for n, _p, c in cc.select()}
    case = sel[name]
    assert case is not None, "regime %r is empty" % name
    assert cc.regime_pred(name)(case), (name, case)
    run_exact(case, cuda)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.family + "-" + c.describe().replace(" ", "_")) for c in cc.exact_cases("large")])
def test_offsets_beyond_one_gib(case, cuda):
    """x, y (and the residual) between 1 GiB and the 2 GiB guard; data in the first and the last image"""
    for b in case.nbytes():
        assert b == 0 or (1 << 30) < b < (1 << 31), (case, case.nbytes())
    run_exact(case, cuda)


def _accuracy_cases():
    out = []
    for pool in cc.POOLS:
        cases = [c for c in cc.exact_cases(pool) if not c.ks and not c.sliced and not c.head]
        fams = sorted({c.family for c in cases})
        for fam in fams:
            best = max((c for c in cases if c.family == fam), key=lambda c: (c.cin * c.k[0] * c.k[1], c.macs()))
            out.append(pytest.param(best, id=pool.replace(" ", "_") + "-" + fam))
    return out


def run_accuracy(case, cuda):
    """Gaussian operands on the guard-banded buffers against float64, at the project's own tolerances"""
    assert not _FAULTED, "an earlier case ended in a HIP error: nothing more is launched"
    x64, w64, scale, shift, res64 = cc.gauss_operands(case)
    ref = cc.ref64(case, x64, w64, scale, shift, res64)
    ref32 = cc.ref64(case, x64, w64, scale, shift, res64, dtype=torch.float32).double()
    D, imap = cc.image_map(case)
    S = float(ref.abs().max())
    tol = (1e-4 + 1e-4 * ref.abs()) if case.path == "f32" else (ref.abs() / 128 + 2e-5 * S)
    torch_ratio = float(((ref32 - ref).abs() / tol).max())
    if torch_ratio > 1.0 / 3:
        tol = 3 * (ref32 - ref).abs().max() + 0 * tol
    x, y, res = _buffers(case, cuda)
    x.load(x64, imap)
    if case.res == 1:
        res.load(res64, imap)
    _load_prior(case, y, res64, imap)
    run, ran = _launcher(case, w64, scale, shift, cuda)
    _assert_ran(case, ran(x, y, res))
    run(x, y, res)
    _sync()
    y.check_untouched(repr(case))
    got = y.body[..., :case.cout + y.off][..., y.off:].double().cpu()
    want = ref.permute(0, 2, 3, 1)[torch.tensor(imap)]
    tolm = tol.permute(0, 2, 3, 1)[torch.tensor(imap)] if tol.dim() == 4 else tol
    ratio = float(((got - want).abs() / tolm).max())
    print("accuracy %-8s %-60s worst error / bound %.3f   torch fp32 / bound %.3f" % (case.family, case.describe(), ratio, torch_ratio))
    assert ratio <= 1.0, (case, ratio)      # NaN fails too


@pytest.mark.parametrize("case", _accuracy_cases())
def test_accuracy(case, cuda):
    """Gaussian operands on the guard-banded buffers against float64, at the project's own tolerances"""
    run_accuracy(case, cuda)


# ---------------------------------------------------------------- the 2 GiB guard
def _refused(case, device, which):
    """the entry point refuses a launch whose x or y byte count is just above 2 GiB and leaves the NaN-filled y untouched; both
    buffers really are that large, so that nothing could leave an allocation if the guard were missing"""
    assert not _FAULTED, "an earlier case ended in a HIP error: nothing more is launched"
    lib = _lib.load()
    for b, big in zip(case.nbytes()[:2], which):
        assert (b > (1 << 31)) == big and b < (1 << 31) + (1 << 28), (case, case.nbytes())
    x64, w64, scale, shift, _ = cc.int_operands(case)
    x, y, _res = _buffers(case, device)
    y.flat.fill_(float("nan"))
    run, _ran = _launcher(case, w64, scale, shift, device)
    with pytest.raises(RuntimeError, match="2 GiB"):
        run(x, y, None)
    _sync()
    assert bool(torch.isnan(y.flat).all()), "%r: y was written although the launch was refused" % (case,)
    assert b"2 GiB" in lib.w2l_last_error()


def test_refuses_a_strided_layer_whose_output_bytes_cross_two_gib(cuda):
    """fp32, 3x3 stride 2: 147456 output pixels, far below any pixel limit - the wide channel stride of y crosses 2 GiB, x stays below"""
    case = cc.Case("f32", "igemm", 0, 8, 72, 3, 2, 1, 0, 4096, 12, 12, force=1, wide=3664, x_wide=512, seed=990)
    _refused(case, cuda, (False, True))


@pytest.mark.parametrize("family", ["igemm", "stem", "box64", "tp2b"])
def test_bf16_families_refuse_above_two_gib(family, cuda):
    case = {"igemm": cc.Case("bf16", "igemm", 0, 8, 72, 3, 1, 1, 0, 4096, 12, 12, force=3, wide=1856, seed=991),
            "stem": cc.Case("bf16", "stem", 0, 6, 16, 7, 1, 3, 0, 4200, 16, 16, wide=1000, seed=992),
            "box64": cc.Case("bf16", "box64", 0, 64, 64, 3, 1, 1, 0, 4200, 16, 16, wide=1000, seed=993),
            "tp2b": cc.Case("bf16", "tp2b", 1, 32, 32, 3, 2, 1, 1, 16384, 5, 7, wide=472, seed=994)}[family]
    if family != "igemm":      # the shape the special-case kernel takes at a dense stride; the guard sits in front of the dispatch
        dense = cc.Case("bf16", family, case.tr, case.cin, case.cout, case.k, case.s, case.p, case.op, case.N // 2, case.H, case.W)
        assert dense.convb_resolve()[0].startswith(family)
    _refused(case, cuda, (True, True))


def main():
    ran = None
    if torch.cuda.is_available():
        dev, ran = torch.device("cuda:0"), {}
        for name, _pool, case in cc.select():
            if case is not None:
                fam, cid, ks, _fl = run_exact(case, dev)
                ran[name] = "%s%s%s" % (fam, " %d" % cid if cid >= 0 else "", " ks %d" % ks if ks > 1 else "")
                if case.path == "bf16" and case.ks:      # not reported by the launcher: the test's restatement of its K-steps
                    ran[name] += " (forced split-K %d: %d splits by the test's own model, unchecked)" % (case.ks, case.splits()[0])
    print(cc.table(ran))
    for c in cc.exact_cases("large"):
        print("  large offsets: %-55s x %.2f GiB  y %.2f GiB  res %.2f GiB" % ((repr(c),) + tuple(b / 2.0 ** 30 for b in c.nbytes())))


if __name__ == "__main__":
    main()
