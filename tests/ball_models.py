"""TEST INFRASTRUCTURE: two small models with ball joints, as XML strings
(ia.Model.from_string loads them; neither is a bundled model, so both run the
generic kernels: static_id() == 0).

  ballarm    fixed base over a floor; ball shoulder (first joint of the tree, on
             a body with a non-identity quat, joint pos off the body origin),
             hinge elbow, ball wrist (anchor and axes carried by the shoulder and
             the elbow), hinge finger (its axis carried by both balls).  Motors
             on the two hinges.  nq 10, nv 8, nu 2.  The arm is 0.95 long and
             hangs 0.6 above the floor: the fore-arm capsule, the hand sphere and
             the finger capsule reach it.  Body geoms collide with the floor
             only (contype 1, conaffinity 0), so a contact state is what its
             name says and nothing else.
  floatarm   a free-floating trunk carrying a ball-jointed limb with a hinge
             below it: the free joint's quaternion and the ball's in one body
             chain.  nq 12, nv 10, nu 1.
"""
import io

BALLARM_XML = """<mujoco model="ballarm">
  <compiler angle="radian" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom condim="3" friction="0.7" margin="0.001" contype="1" conaffinity="0"/></default>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 0.1" contype="1" conaffinity="1"/>
    <body name="upper" pos="0 0 0.6" quat="0.9 0.1 0.3 -0.2">
      <joint name="shoulder" type="ball" pos="0.02 -0.01 0.03" armature="0.02" damping="0.3"/>
      <geom name="cupper" type="capsule" fromto="0 0 0 0.3 0 0" size="0.04"/>
      <body name="fore" pos="0.3 0 0">
        <joint name="elbow" type="hinge" axis="0 1 0" pos="0 0 0.01" limited="true" range="-2.2 2.2" armature="0.01"
               damping="0.1"/>
        <geom name="cfore" type="capsule" fromto="0 0 0 0.3 0.02 0" size="0.035"/>
        <body name="hand" pos="0.3 0.02 0" quat="0.95 -0.2 0.1 0.15">
          <joint name="wrist" type="ball" pos="0.01 0 -0.01" armature="0.01" damping="0.15"/>
          <geom name="shand" type="sphere" pos="0.08 0 0" size="0.06"/>
          <body name="finger" pos="0.13 0 0">
            <joint name="knuckle" type="hinge" axis="0 0 1" armature="0.005" damping="0.05"/>
            <geom name="cfinger" type="capsule" fromto="0 0 0 0.18 0 0" size="0.02"/>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor joint="elbow" gear="8" ctrllimited="true" ctrlrange="-1 1"/>
    <motor joint="knuckle" gear="2"/>
  </actuator>
</mujoco>"""

FLOATARM_XML = """<mujoco model="floatarm">
  <compiler angle="radian" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom condim="3" friction="0.8" margin="0.001"/></default>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 0.1"/>
    <body name="trunk" pos="0 0 1.0" quat="0.8 0.2 -0.4 0.4">
      <freejoint name="root"/>
      <geom name="ctrunk" type="capsule" fromto="-0.15 0 0 0.15 0 0" size="0.07"/>
      <body name="thigh" pos="0.15 0 -0.05" quat="0.9 0.3 0.1 0.3">
        <joint name="hip" type="ball" pos="0 0.01 0.02" armature="0.02" damping="0.2"/>
        <geom name="cthigh" type="capsule" fromto="0 0 0 0 0 -0.3" size="0.04"/>
        <body name="shin" pos="0 0 -0.3">
          <joint name="knee" type="hinge" axis="0 1 0" limited="true" range="-2.4 0.1" armature="0.01" damping="0.1"/>
          <geom name="cshin" type="capsule" fromto="0 0 0 0.02 0 -0.25" size="0.035"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor joint="knee" gear="10" ctrllimited="true" ctrlrange="-1 1"/>
  </actuator>
</mujoco>"""

BALL_XML = {"ballarm": BALLARM_XML, "floatarm": FLOATARM_XML}
BALL_SIZES = {"ballarm": (10, 8, 2), "floatarm": (12, 10, 1)}   # nq, nv, nu


def ball_file(name):
    """an open file of the model's XML, for tests/mjcf_indep.compile_mjcf"""
    return io.StringIO(BALL_XML[name])


def ball_model(ia, name):
    """the product's compile of the model; the generic kernels are what runs it"""
    m = ia.Model.from_string(BALL_XML[name])
    assert (m.nq, m.nv, m.nu) == BALL_SIZES[name]
    assert m.static_id() == 0
    return m


def ball_quat_slices(C):
    """[(qpos address, dof address)] of every ball joint of an mjcf_indep model"""
    out, aq, ad = [], 0, 0
    for j in C.joints:
        if j["type"] == "ball":
            out.append((aq, ad))
        aq += {"free": 7, "ball": 4}.get(j["type"], 1)
        ad += {"free": 6, "ball": 3}.get(j["type"], 1)
    return out
