// group_linear_store.inc — included by the two channel-major kernels of group_linear.hip where one channel's four outputs leave:
// v (float4) is rounded to the stored type OT, stored at o, and the thread's sums s / ss advance by the STORED values.
// Text, not a function: as a forced-inline function (v by value or by reference) the block moved the VGPRs of
// group_linear_fwd_kernel<bf16> (38 -> 40) and of group_linear_direct_kernel<.., 1> (profiles/group_shared_pieces.txt).
            if constexpr (sizeof(OT) == 2) {
                v.x = ogc_as_stored<OT>(v.x); v.y = ogc_as_stored<OT>(v.y); v.z = ogc_as_stored<OT>(v.z); v.w = ogc_as_stored<OT>(v.w);
            }
            ogc_st4(o, v);
            s += (v.x + v.y) + (v.z + v.w);
            ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
