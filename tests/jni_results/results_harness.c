/*
 * results_harness.c -- the processResultAcks native of integration/owgs_jni.c executed without a JVM
 * (tests/test_gpu_result_acks_jni.py).
 *
 * The JNIEnv stand-in, its Java-object stand-ins and the ctypes surface for creating objects and contexts are
 * tests/jni_stub/jni_harness.c's, compiled into this library unchanged by including it; only the h_* wrapper below is
 * new.  integration/Makefile builds it as integration/build/libowgs_jni_results_harness.so.
 */
#include "../jni_stub/jni_harness.c"

jint JN(processResultAcks)(JNIEnv*, jobject, jlong, jbyteArray, jlongArray, jint, jbyteArray, jintArray, jintArray,
                           jbyteArray, jlongArray, jlongArray, jintArray, jlong, jint, jintArray);

HX int32_t h_process_result_acks(int64_t h, void* bytes, void* off, int32_t n, void* out_kind, void* out_invoker,
                                 void* out_ticket, void* out_flags, void* out_aid, void* out_resp_off,
                                 void* out_resp_len, int64_t now_ms, int32_t apply, void* out_summary) {
    return JN(processResultAcks)(&g_env, NULL, h, bytes, off, n, out_kind, out_invoker, out_ticket, out_flags, out_aid,
                                 out_resp_off, out_resp_len, now_ms, apply, out_summary);
}
