/*
 * feeds_harness.c -- the supervision-feed natives of integration/owgs_jni.c (processPings, processAcksSupervised,
 * completeActivationsSupervised) executed without a JVM (tests/test_gpu_feeds_jni.py).
 *
 * The JNIEnv stand-in, its Java-object stand-ins and the ctypes surface for creating objects and contexts are
 * tests/jni_stub/jni_harness.c's, compiled into this library unchanged by including it; only the three h_* wrappers
 * below are new.  integration/Makefile builds it as integration/build/libowgs_jni_feeds_harness.so.
 */
#include "../jni_stub/jni_harness.c"

jint JN(processPings)(JNIEnv*, jobject, jlong, jbyteArray, jlongArray, jlongArray, jint, jlong, jint, jbyteArray,
                      jintArray, jlongArray, jintArray);
jint JN(processAcksSupervised)(JNIEnv*, jobject, jlong, jbyteArray, jlongArray, jint, jbyteArray, jintArray, jintArray,
                               jbyteArray, jlong, jint, jintArray);
jint JN(completeActivationsSupervised)(JNIEnv*, jobject, jlong, jbyteArray, jintArray, jbyteArray, jint, jbyteArray,
                                       jintArray, jbyteArray, jlong, jint, jintArray);

HX int32_t h_process_pings(int64_t h, void* bytes, void* off, void* t_ms, int32_t n, int64_t now_ms, int32_t apply,
                           void* out_kind, void* out_instance, void* out_mem, void* out_summary) {
    return JN(processPings)(&g_env, NULL, h, bytes, off, t_ms, n, now_ms, apply, out_kind, out_instance, out_mem,
                            out_summary);
}
HX int32_t h_process_acks_supervised(int64_t h, void* bytes, void* off, int32_t n, void* out_kind, void* out_invoker,
                                     void* out_ticket, void* out_flags, int64_t now_ms, int32_t apply,
                                     void* out_summary) {
    return JN(processAcksSupervised)(&g_env, NULL, h, bytes, off, n, out_kind, out_invoker, out_ticket, out_flags,
                                     now_ms, apply, out_summary);
}
HX int32_t h_complete_activations_supervised(int64_t h, void* aid32, void* invokers, void* flags, int32_t n,
                                             void* out_kind, void* out_ticket, void* out_flags, int64_t now_ms,
                                             int32_t apply, void* out_summary) {
    return JN(completeActivationsSupervised)(&g_env, NULL, h, aid32, invokers, flags, n, out_kind, out_ticket,
                                             out_flags, now_ms, apply, out_summary);
}
