/*
 * events_harness.c -- the throttle-gate event natives of integration/owgs_jni.c (setEventSource,
 * registerEventIdentities, invokeActivationsEvents) executed without a JVM (tests/test_gpu_events_jni.py).
 *
 * The JNIEnv stand-in, its Java-object stand-ins and the ctypes surface for creating objects and contexts are
 * tests/jni_stub/jni_harness.c's, compiled into this library unchanged by including it; only the h_* wrappers below
 * are new.  integration/Makefile builds it as integration/build/libowgs_jni_events_harness.so.
 */
#include "../jni_stub/jni_harness.c"

jint JN(setEventSource)(JNIEnv*, jobject, jlong, jbyteArray);
jint JN(registerEventIdentities)(JNIEnv*, jobject, jlong, jbyteArray, jlongArray, jbyteArray, jlongArray, jint);
jint JN(invokeActivationsEvents)(JNIEnv*, jobject, jlong, jobject, jobject, jobject, jobject, jint, jlong, jlong, jlong,
                                 jlong);

HX int32_t h_set_event_source(int64_t h, void* json) { return JN(setEventSource)(&g_env, NULL, h, json); }

HX int32_t h_register_event_identities(int64_t h, void* a, void* a_off, void* b, void* b_off, int32_t n) {
    return JN(registerEventIdentities)(&g_env, NULL, h, a, a_off, b, b_off, n);
}

HX int32_t h_invoke_activations_events(int64_t h, void* in, void* out, void* ev_in, void* ev_out, int32_t n,
                                       int64_t ev_cap, int64_t rej_cap, int64_t seq_base, int64_t now_ms) {
    return JN(invokeActivationsEvents)(&g_env, NULL, h, in, out, ev_in, ev_out, n, ev_cap, rej_cap, seq_base, now_ms);
}
