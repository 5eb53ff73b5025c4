/*
 * rg_stream.h -- the counter-based random stream of librg_mpc.so, stated once.  Every unit that draws (the episode reset's
 * targets, the random terrain and through it the height scan, the policy and OU noise, the DDPG sampler, the domain
 * randomiser, the sensor model, the estimator model) draws from it, and the header of each says which words it chains and
 * what it does with the result.  There is no state and no entry point: a draw is a function of a seed and a few 64-bit words,
 * so it does not depend on who else draws, in which order, or on the batch.  On the device it is
 * robot_gym_amd/csrc/rg_stream_dev.inc, in numpy tests/stream_model.py; tests/test_stream_cpu.py pins known answers.
 *
 * mix.  All arithmetic is uint64 and wraps:
 *      mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   (the finaliser of SplitMix64: mix(0x9E3779B97F4A7C15) = 0xE220A8397B1DCDAF is that generator's first output from seed 0).
 *
 * The chain over N words w1 .. wN:
 *      h = seed;  for w in (w1, .., wN):  h = mix((h ^ w) + 0x9E3779B97F4A7C15)
 *   A signed word enters as its two's-complement 64-bit pattern.  `hash(w1, .., wN)` below is this h.
 *
 * u.  The 53-bit uniform of a chain:
 *      u(w1, .., wN) = (hash(w1, .., wN) >> 11) * 2^-53                                        in [0, 1)
 *
 * ix.  The index word of a per-tick draw:
 *      ix(k, row, j) = (k << 12) | (row << 2) | j        (uint64; k the robot's tick counter, row < 1024, j in 0..3)
 *   k is at most 2^52 (below), where k << 12 wraps to 0.
 *
 * n.  A unit-variance noise draw takes four hashes:
 *      n(key, draw, purpose, k, row) = (((u0 + u1) + (u2 + u3)) - 2.0) * 1.7320508075688772,   uj = u(key, draw, purpose, ix(k, row, j))
 *   This is an Irwin-Hall sum of four uniforms, centred and scaled to variance 1 (4 / 12 * 3), NOT a Gaussian: |n| < 3.4642
 *   (2 * sqrt 3), and its fourth moment is 2.7, not 3.  A Gaussian needs log and cos (or an inverse error function), whose
 *   device and host implementations differ in the last bits; four additions are correctly rounded everywhere, and that is
 *   what keeps the models that use n bit-exact.  (The policy noise of rg_policy.h IS a Gaussian, and pays that price.)
 *
 * The two integer readings of a state row (a double the caller owns):
 *      word_of(v)     = (uint64) (int64) v                      a key, a draw count, an episode count: any sign
 *      bounded(v, hi) = (uint64) fmin(fmax(v, 0), hi)           a tick, delay or run row the caller may have written; a NaN is 0
 *   A tick row is read as bounded(v, 2^52).
 *
 * Registry: who chains which words.
 *   Streams keyed (key, draw, purpose, index), one per robot and episode; the purpose word keeps their draws apart, so a seed
 *   and a key shared between them do not correlate them.  Each user owns a block of 16 purposes and defines them in its own
 *   header:
 *      block 0   0..15   rg_dr.h       0 mass, 1 inertia, 2 world, 3 push start, 4 push component, 5 push gate
 *      block 1  16..31   rg_sensor.h  16 observation delay, 17 action delay, 18 bias, 19 observation noise, 20 dropout, 21 action noise
 *      block 2  32..47   rg_est.h     32 bias, 33 noise, 34 contact miss, 35 contact ghost
 *      block 3  48..63   rg_srb_friction.h  48 friction coefficient
 *      block 4  64..79   rg_srb_motor.h     64 motor strength (the index word is the motor)
 *   A NEW USER TAKES THE NEXT FREE BLOCK OF 16 (block 5, 80..95); a user that needs a new purpose takes the next free one of its
 *   own block.  Each unit asserts at compile time that its purposes lie in its block, and the test that their values are
 *   pairwise disjoint.
 *   Streams with words of their own, which have no purpose word (a different chain position by meaning; give them a seed of
 *   their own where that matters):
 *      rg_episode.h  target         (key, episode, attempt, axis)
 *      rg_srb.h      terrain        (key, I, J)                      also read by rg_srb_contact.h and rg_scan.h
 *      rg_policy.h   policy noise   (key, counter, axis, draw)       also rg_rnn.h and rg_ddpg.h's OU noise
 *      rg_ddpg.h     sampler        (updates, m, draw)
 */
#ifndef RG_STREAM_H
#define RG_STREAM_H
#endif
