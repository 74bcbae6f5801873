/*
 * invoke_harness.c -- the invokeActivations native of integration/owgs_jni.c executed without a JVM
 * (tests/test_gpu_invoke_jni.py).
 *
 * The JNIEnv stand-in, its Java-object stand-ins and the ctypes surface for creating objects and contexts are
 * tests/jni_stub/jni_harness.c's, compiled into this library unchanged by including it; only the h_* wrapper below is
 * new.  integration/Makefile builds it as integration/build/libowgs_jni_invoke_harness.so.
 */
#include "../jni_stub/jni_harness.c"

jint JN(invokeActivations)(JNIEnv*, jobject, jlong, jobject, jobject, jint, jlong, jlong);

HX int32_t h_invoke_activations(int64_t h, void* in, void* out, int32_t n, int64_t seq_base, int64_t now_ms) {
    return JN(invokeActivations)(&g_env, NULL, h, in, out, n, seq_base, now_ms);
}
