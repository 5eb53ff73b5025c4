// rg_reset_body.inc -- LocomotionController.reset for one robot, as statements: the body of rg_reset_kernel (rg_mpc.hip) and
// of the masked reset (rg_episode.hip).  Included inside a kernel with these names in scope: c (const DevCfg *), st
// (DevState), b (the robot), B (the batch) and the macro RG_RESET_T0 (the robot's clock value at the reset).
  st.reset_time[b] = RG_RESET_T0;
  st.flags[b] = 3;
  int ld = 0;
  for (int l = 0; l < 4; l++) ld |= ((st.g_init ? st.g_init[l * B + b] : c->init_state[l]) & 1) << l;
  st.last_desired[b] = ld;
  st.ring_len[b] = 0; st.ring_head[b] = 0;
  for (int a = 0; a < 3; a++) { st.fsum[a * B + b] = 0.0; st.fcorr[a * B + b] = 0.0; }
  st.swing_valid[b] = 0;
  st.warm_key[b] = -1;
  st.hard[b] = 0;    // a reset robot is a fresh robot: ADMM first, no direct routing, no cost prediction from before
  st.iters[b] = 0;
