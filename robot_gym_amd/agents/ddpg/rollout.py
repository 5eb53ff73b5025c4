"""DDPG's one continuing stream of experience on the device: the collector (act, step, store, update) and the deterministic
player.  Nothing here reads device data on the host: every tick is kernel launches on the current stream."""
import torch


def collect(env, agent, ticks, updates_per_tick=1, warmup=50):
    """`ticks` steps of `env` (a BatchedGoEnv after reset(), with auto_reset: DDPG learns from one continuing stream, a frozen
    robot would fill the ring with a dead transition per tick) under `agent`.  Per tick: the observation into a slot of the
    agent's; act with OU noise; env.step; store; then updates_per_tick updates once the agent has stored `warmup` ticks (the
    reference's nb_steps_warmup_actor / _critic = 50).  Returns agent.stats (a device tensor)."""
    if not getattr(env, "auto_reset", False):
        raise ValueError("collect: the environment must be made with auto_reset=True")
    if int(env.batch) != agent.batch:
        raise ValueError(f"collect: env.batch is {env.batch}, the agent's batch is {agent.batch}")
    slot, action = agent._obs_slot, agent._action
    with torch.no_grad():
        for _ in range(int(ticks)):
            slot.copy_(env.obs.t())   # the step overwrites the environment's buffer; the slot is what act and store read
            agent.act(slot, noise=True, out=dict(action=action))
            _, reward, done = env.step(action)
            agent.store(slot, action, reward, done)
            if updates_per_tick > 0 and agent.ticks_stored >= warmup:
                agent.update(updates_per_tick)
    return agent.stats


def play(env, agent, ticks):
    """The deterministic player: `ticks` steps of action = actor(window), no noise, no update.  Every tick is stored, since the
    window is read from the ring: play on agent.clone() to keep greedy ticks out of a ring that is still learnt from.  Returns
    the sum of the rewards per robot, a device tensor [B]."""
    total = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
    slot, action = agent._obs_slot, agent._action
    with torch.no_grad():
        for _ in range(int(ticks)):
            slot.copy_(env.obs.t())
            agent.act(slot, noise=False, out=dict(action=action))
            _, reward, done = env.step(action)
            agent.store(slot, action, reward, done)
            total += reward
    return total
