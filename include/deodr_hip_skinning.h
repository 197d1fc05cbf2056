/* include/deodr_hip_skinning.h -- companion header of include/deodr_hip.h: linear blend skinning (a skeleton, skin weights) on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_SKINNING_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE MODEL.  J joints with rest positions joints [J,3] and parents [J]; joint 0 is the root, parents[j] < j for j > 0.  One quaternion per pose
 * and joint, quaternions [n,J,4] = (x, y, z, w), normalised inside (the adjoint goes through q / |q|, as deodr_hip_fit_pose_project does for the view
 * poses).  With R(q) the rotation of a unit quaternion, world transforms of pose b:
 *     root:   R_0 = R(q_0)          t_0 = joints_0
 *     other:  R_j = R_p R(q_j)      t_j = t_p + R_p (joints_j - joints_p)        p = parents[j]
 * and the skinned vertices, indices and weights [V,K] (rows with fewer than K influences padded with weight 0):
 *     posed[b,i] = sum_k weights[i,k] (R_j (vertices[i] - joints_j) + t_j)        j = indices[i,k]
 * With every quaternion at identity posed == vertices up to rounding wherever the weights of a row sum to 1.
 * world [n,J,7] holds (Q_j, t_j): R_j as the composed unit quaternion Q_j = Q_p (q_j / |q_j|) (Hamilton product), then t_j.
 *
 * THE TABLES.  parents, indices and the transposed table are device arrays of uint32.  parents[0] is ignored: joint 0 is the root, and so is any
 * j > 0 with parents[j] >= j (0xFFFFFFFF is the customary marker).  The transposed table lists, joint by joint, the slots s = i K + k of the
 * influences (vertex i, column k) with indices[i,k] = j: joint_offsets [J+1] (non-decreasing, joint_offsets[J] = nnz) and joint_slots [nnz],
 * 0 <= nnz <= V K.  The order of a joint's slots is the order its sums are taken in.  Influences left out of the table (weight 0) add nothing.
 * An entry out of range is never dereferenced: an indices[i,k] >= J counts as weight 0, a joint_slots entry >= V K is skipped, offsets are clamped to
 * nnz.  (A transposed table that does not match indices gives sums over the wrong influences, not a fault.)
 *
 * CONTRACT
 *   - vertices, joints, quaternions, weights, world, posed and every adjoint are contiguous float64, 8-byte aligned; the uint32 arrays 4-byte aligned.
 *   - Double arithmetic, no atomics: the order of every sum is fixed by the tables and (V, J, K, n) alone, so results are bit-identical from run to
 *     run and do not depend on which optional outputs are asked for.
 *   - Limits: 1 <= n <= 64, 1 <= J <= 256, 1 <= K <= 8, 1 <= V <= 2^24.
 *   - Refused before any launch, with a message: a NULL among the required pointers, no output requested, a value outside the limits, a misaligned
 *     pointer, scratch_bytes below deodr_hip_skin_scratch_bytes, an output that overlaps an input, the scratch or another output.
 */
#ifndef DEODR_HIP_SKINNING_H
#define DEODR_HIP_SKINNING_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two launches: the chain (one workgroup; thread b walks the joints of pose b in order) -> world [n,J,7]; then grid (ceil(8 V / 256), n), eight
 * adjacent lanes per vertex, one influence each -> posed [n,V,3].  Both outputs are required. */
int deodr_hip_skin_apply(const double *vertices, const double *joints, const uint32_t *parents, const double *quaternions, const uint32_t *indices,
						 const double *weights, double *world, double *posed, int V, int J, int K, int n, void *stream);

/* The adjoint for posed_b [n,V,3]; world is what deodr_hip_skin_apply wrote for the same inputs.  Outputs, each may be NULL but not all:
 *   vertices_b [V,3]:      sum over poses (in order) and influences of weights[i,k] R_j^T posed_b[b,i]; one launch, eight lanes per vertex.
 *   quaternions_b [n,J,4]: with respect to the raw quaternions.
 *   joints_b [J,3]:        summed over the poses in pose order by one thread per element.
 * quaternions_b and joints_b take two launches: grid (J, n), the workgroup of (joint, pose) strides the joint's slots -- thread t of 256 takes entries
 * t, t + 256, ..; threads -> lanes -> wavefronts in order --; then one workgroup walks the joints of every pose from the last to the first.
 * scratch: device memory of deodr_hip_skin_scratch_bytes(V, J, K, n) bytes, 8-byte aligned, used by one stream at a time; it need not be cleared.
 * The scratch after a call that asked for quaternions_b or joints_b (part of this ABI version): 64 bytes that are not touched, then [n,J,10] doubles:
 * the adjoints of Q_j (4) and t_j (3) of world with everything the joints below j passed up, and pose b's share of joints_b[j] (3). */
int deodr_hip_skin_apply_b(const double *vertices, const double *joints, const uint32_t *parents, const double *quaternions, const uint32_t *indices,
						   const double *weights, const double *world, const double *posed_b, const uint32_t *joint_offsets,
						   const uint32_t *joint_slots, int nnz, double *vertices_b, double *quaternions_b, double *joints_b, void *scratch,
						   size_t scratch_bytes, int V, int J, int K, int n, void *stream);

/* Bytes of scratch deodr_hip_skin_apply_b needs (64 + 80 n J); 0 outside the limits above. */
size_t deodr_hip_skin_scratch_bytes(int V, int J, int K, int n);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_skinning_abi_version(void);
#define DEODR_HIP_SKINNING_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SKINNING_H */
